// Analytic acquisition on the posterior predictive of an equal-weight mixture of P Gaussians per candidate, with a fused argmax.
//   pacoh_mixture_acq   per task t and candidate j of mu, var [T*P, m] (the output of pacoh_gp_cond_predict / pacoh_gp_predict): the
//                       value of 'ei' / 'pi' / 'ucb' / 'mean' / 'std' by the rule of meta_learning_pacoh_amd/acquisition.py
//                       (mixture_acquisition: the same operations in the same order, nothing contracted to an fma), optionally
//                       written to values [T,m], and per task the eligible candidate with the greatest / smallest value by the
//                       selection rule of pacoh_gp_path_argmax (paths.first_best / merge_best).
// Two launches, no atomics, no waiting: (1) grid = tasks x STRIPS of consecutive 256-point blocks; a thread owns the points
// lo + tid + 256 i of its strip in ascending order, walks the P rows of each (coalesced across the block), keeps its running
// (value, index) pair, then the block reduces the 256 pairs by (value, smaller index) -- six shuffle steps per wave, four pairs
// through LDS -- and writes ONE partial pair per (task, strip); (2) a wave per task merges the strips and, with first = 0, the pair
// already in best_*.  The merge is the one of gp_path.hip in spirit; its few lines are duplicated here, not shared across files.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "pacoh_gp.h"

namespace pacoh {
namespace {

constexpr int ANT = 256;                 // threads of a workgroup = points of a block
constexpr int ARB = 4;                   // parameter rows whose moments a thread loads at once

template <typename T> __device__ __forceinline__ T t_erfc(T x);
template <> __device__ __forceinline__ float t_erfc<float>(float x) { return erfcf(x); }
template <> __device__ __forceinline__ double t_erfc<double>(double x) { return erfc(x); }

template <typename T> __device__ __forceinline__ T acq_shfl_xor(T x, int d);
template <> __device__ __forceinline__ float acq_shfl_xor<float>(float x, int d) { return __shfl_xor(x, d, 64); }
template <> __device__ __forceinline__ double acq_shfl_xor<double>(double x, int d) { return __shfl_xor(x, d, 64); }

template <typename T>
struct AcqArgs {
    const T* mu; const T* var;          // [T][P][m]
    const T* noise;                     // [P] | NULL
    const uint8_t* mask;                // [m] | NULL
    T* values;                          // [T][m] | NULL
    int64_t* part_idx; T* part_val;     // [T][strips]
    T* best_val; int64_t* best_idx;     // [T]
    T best, xi, sb;                     // sb = sign * beta
    int64_t idx_base;
    int sign, Tn, P, m, nblk, strips, largest, first;
};

// is the pair (vb, ib) ahead of (va, ia)?  idx < 0 marks "nothing"; values of pairs with idx >= 0 are never NaN
template <typename T, typename I>
__device__ __forceinline__ bool acq_ahead(T va, I ia, T vb, I ib, int largest) {
    if (ib < 0) return false;
    if (ia < 0) return true;
    if (vb == va) return ib < ia;
    return largest ? vb > va : vb < va;
}

// the rule at one candidate: mu, var point at row 0 of the task, column j; rows are m apart
template <typename T, int KIND>
__device__ __forceinline__ T acq_point(const AcqArgs<T>& a, const T* __restrict__ mu, const T* __restrict__ var) {
#pragma clang fp contract(off)
    const long m = a.m;
    const T sgn = T(a.sign);
    T M = T(0), S = T(0), V = T(0), acc = T(0);
    // the rows are walked in order, ARB at a time: their loads are issued together (a row past the end reads row p0 again, unused),
    // so that a thread waits for memory once per ARB rows and not once per row -- there are too few waves to hide that wait
    for (int p0 = 0; p0 < a.P; p0 += ARB) {
        T ub[ARB], vb[ARB];
#pragma unroll
        for (int i = 0; i < ARB; ++i) {
            const long o = (p0 + i < a.P ? p0 + i : p0) * m;
            ub[i] = mu[o];
            vb[i] = KIND == PACOH_ACQ_MEAN ? T(0) : var[o];
        }
#pragma unroll
        for (int i = 0; i < ARB; ++i) {
            const int p = p0 + i;
            if (p >= a.P) break;                                         // (uniform)
            const T u = ub[i];
            T v = vb[i];
            if (KIND != PACOH_ACQ_MEAN) {
                if (a.noise) v -= a.noise[p];
                v = v < T(0) ? T(0) : v;
            }
            if (KIND == PACOH_ACQ_MEAN || KIND == PACOH_ACQ_STD || KIND == PACOH_ACQ_UCB) {
                const T k = T(p + 1);
                const T dl = u - M;
                M += dl / k;
                if (KIND != PACOH_ACQ_MEAN) {
                    S += dl * (u - M);
                    V += (v - V) / k;
                }
            } else {
                const T d = sgn * (u - a.best) - a.xi;
                const T s = t_sqrt<T>(v);
                T term;
                if (s > T(0)) {
                    const T z = d / s;
                    const T Phi = T(0.5) * t_erfc<T>(-z / T(1.41421356237309504880));
                    if (KIND == PACOH_ACQ_PI) {
                        term = Phi;
                    } else {
                        const T phi = t_exp<T>(-(z * z) / T(2)) / T(2.50662827463100050242);
                        const T e = s * (z * Phi + phi);
                        term = e < T(0) ? T(0) : e;                      // (a NaN stays NaN)
                    }
                } else if (s == T(0)) {
                    if (KIND == PACOH_ACQ_PI) term = d > T(0) ? T(1) : (d == d ? T(0) : d);
                    else term = d < T(0) ? T(0) : d;
                } else {
                    term = T(NAN);
                }
                acc += term;
            }
        }
    }
    if (KIND == PACOH_ACQ_MEAN) return M;
    if (KIND == PACOH_ACQ_STD || KIND == PACOH_ACQ_UCB) {
        const T sd = t_sqrt<T>(V + S / T(a.P));
        return KIND == PACOH_ACQ_STD ? sd : M + a.sb * sd;
    }
    return acc / T(a.P);
}

template <typename T, int KIND>
__global__ void __launch_bounds__(ANT) mixture_acq_kernel(AcqArgs<T> a) {
    __shared__ T wv[ANT / 64];
    __shared__ int wi[ANT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int strip = (int)blockIdx.x;
    const long t = blockIdx.y;
    const long m = a.m;
    const int blk_lo = (int)((long)strip * a.nblk / a.strips), blk_hi = (int)((long)(strip + 1) * a.nblk / a.strips);
    const T* mu = a.mu + t * a.P * m;
    const T* var = a.var + t * a.P * m;
    T run_v = T(NAN);
    int run_j = -1;
    for (int blk = blk_lo; blk < blk_hi; ++blk) {
        const long j = (long)blk * ANT + tid;
        if (j < m) {
            const T val = acq_point<T, KIND>(a, mu + j, var + j);
            if (a.values) a.values[t * m + j] = val;
            const bool ok = val == val && (!a.mask || a.mask[j] != 0);
            // (two selects on one condition, not a branch: value and index always move together)
            const bool better = a.largest ? val > run_v : val < run_v;
            const bool take = ok & ((run_j < 0) | better);
            run_v = take ? val : run_v;
            run_j = take ? (int)j : run_j;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const T ov = acq_shfl_xor<T>(run_v, d);
        const int oj = __shfl_xor(run_j, d, 64);
        const bool take = acq_ahead<T, int>(run_v, run_j, ov, oj, a.largest);
        run_v = take ? ov : run_v;
        run_j = take ? oj : run_j;
    }
    if (lane == 0) { wv[wave] = run_v; wi[wave] = run_j; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < ANT / 64; ++w) {
            const bool take = acq_ahead<T, int>(run_v, run_j, wv[w], wi[w], a.largest);
            run_v = take ? wv[w] : run_v;
            run_j = take ? wi[w] : run_j;
        }
        const long o = t * a.strips + strip;
        a.part_val[o] = run_v;
        a.part_idx[o] = run_j < 0 ? (int64_t)-1 : a.idx_base + run_j;
    }
}

template <typename T>
__global__ void __launch_bounds__(ANT) mixture_acq_merge_kernel(AcqArgs<T> a) {
    const int lane = threadIdx.x & 63;
    const long t = (long)blockIdx.x * (ANT / 64) + (threadIdx.x >> 6);
    if (t >= a.Tn) return;                           // (uniform per wave)
    T bv = T(NAN);
    int64_t bi = -1;
    for (int st = lane; st < a.strips; st += 64) {
        const T v = a.part_val[t * a.strips + st];
        const int64_t i = a.part_idx[t * a.strips + st];
        { const bool take = acq_ahead<T, int64_t>(bv, bi, v, i, a.largest); bv = take ? v : bv; bi = take ? i : bi; }
    }
    if (lane == 0 && !a.first) {
        const T v = a.best_val[t];
        const int64_t i = v == v ? a.best_idx[t] : (int64_t)-1;
        { const bool take = acq_ahead<T, int64_t>(bv, bi, v, i, a.largest); bv = take ? v : bv; bi = take ? i : bi; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const T v = acq_shfl_xor<T>(bv, d);
        const int lo = __shfl_xor((int)(bi & 0xffffffffLL), d, 64), hi = __shfl_xor((int)(bi >> 32), d, 64);
        const int64_t i = ((int64_t)hi << 32) | (uint32_t)lo;
        { const bool take = acq_ahead<T, int64_t>(bv, bi, v, i, a.largest); bv = take ? v : bv; bi = take ? i : bi; }
    }
    if (lane == 0) {
        a.best_val[t] = bi < 0 ? T(NAN) : bv;
        a.best_idx[t] = bi;
    }
}

// partial pairs that strips = 0 aims at: one block per strip where that fits, else ceil(ACQ_GRID / T) strips per task -- the bound
// caps the partials of a very large call (12 - 16 bytes per pair), it is not there to make strips long
constexpr long ACQ_GRID = 32768;

inline long acq_blocks(int m) { return ((long)m + ANT - 1) / ANT; }

// strips of a call: a positive request clamped to the block count; 0: ceil(ACQ_GRID / T), at least 1, at most the block count
inline int acq_strips(int T, int m, int strips) {
    const long want = strips > 0 ? strips : (ACQ_GRID + T - 1) / T;
    return (int)std::max(1L, std::min(want, acq_blocks(m)));
}

// partial pairs the workspace holds: the call's own T strips for a positive request; for strips = 0 the bound
// min(T blocks, ACQ_GRID - 1 + T) >= T strips, which unlike the exact count never shrinks as T grows
inline size_t acq_pairs(int T, int m, int strips) {
    if (strips > 0) return (size_t)T * (size_t)acq_strips(T, m, strips);
    return (size_t)std::min((long)T * acq_blocks(m), ACQ_GRID - 1 + T);
}

template <typename T>
int acq_entry(const void* mu, const void* var, const void* noise, const uint8_t* mask, void* values, void* best_val,
              int64_t* best_idx, void* workspace, int kind, double best, double xi, double beta, int sign, int Tn, int P, int m,
              int64_t idx_base, int largest, int first, int strips, hipStream_t stream) {
    AcqArgs<T> a = {};
    a.mu = (const T*)mu; a.var = (const T*)var; a.noise = (const T*)noise; a.mask = mask; a.values = (T*)values;
    a.best_val = (T*)best_val; a.best_idx = best_idx;
    a.best = (T)best; a.xi = (T)xi; a.sb = (T)((double)sign * beta);
    a.idx_base = idx_base; a.sign = sign; a.Tn = Tn; a.P = P; a.m = m; a.largest = largest; a.first = first;
    a.nblk = (int)acq_blocks(m);
    a.strips = acq_strips(Tn, m, strips);
    a.part_idx = (int64_t*)workspace;                // the 8-byte entries first: both arrays stay aligned
    a.part_val = (T*)(a.part_idx + (long)Tn * a.strips);
    void (*kern)(AcqArgs<T>) = nullptr;
    switch (kind) {
        case PACOH_ACQ_EI: kern = mixture_acq_kernel<T, PACOH_ACQ_EI>; break;
        case PACOH_ACQ_PI: kern = mixture_acq_kernel<T, PACOH_ACQ_PI>; break;
        case PACOH_ACQ_UCB: kern = mixture_acq_kernel<T, PACOH_ACQ_UCB>; break;
        case PACOH_ACQ_MEAN: kern = mixture_acq_kernel<T, PACOH_ACQ_MEAN>; break;
        default: kern = mixture_acq_kernel<T, PACOH_ACQ_STD>; break;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)a.strips, (unsigned)Tn), dim3(ANT), 0, stream, a);
    const int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(mixture_acq_merge_kernel<T>, dim3((unsigned)((Tn + ANT / 64 - 1) / (ANT / 64))), dim3(ANT), 0, stream, a);
    return launch_status();
}

}  // namespace
}  // namespace pacoh

using namespace pacoh;

extern "C" size_t pacoh_mixture_acq_workspace_bytes(int T, int m, int strips, int dtype) {
    if (check_dtype(dtype) || T <= 0 || T > 65535 || m < 1 || strips < 0) return 0;
    return acq_pairs(T, m, strips) * (sizeof(int64_t) + (dtype == PACOH_F32 ? sizeof(float) : sizeof(double)));
}

extern "C" int pacoh_mixture_acq(const void* mu, const void* var, const void* noise, const uint8_t* mask, void* values, void* best_val,
                                 int64_t* best_idx, void* workspace, size_t workspace_bytes, int kind, double best, double xi,
                                 double beta, int sign, int T, int P, int m, int64_t idx_base, int largest, int first, int strips,
                                 int dtype, void* stream) {
    if (check_dtype(dtype)) return PACOH_EDTYPE;
    if (T <= 0 || P <= 0 || m <= 0) return PACOH_EINVAL;
    if (T > 65535) return PACOH_ELIMIT;
    if (kind < PACOH_ACQ_EI || kind > PACOH_ACQ_STD || (sign != 1 && sign != -1)) return PACOH_EINVAL;
    if (strips < 0 || idx_base < 0 || (largest != 0 && largest != 1) || (first != 0 && first != 1)) return PACOH_EINVAL;
    if (!mu || !var || !best_val || !best_idx || !workspace) return PACOH_EINVAL;
    if (workspace_bytes < pacoh_mixture_acq_workspace_bytes(T, m, strips, dtype)) return PACOH_EINVAL;
    if (dtype == PACOH_F32)
        return acq_entry<float>(mu, var, noise, mask, values, best_val, best_idx, workspace, kind, best, xi, beta, sign, T, P, m,
                                idx_base, largest, first, strips, (hipStream_t)stream);
    return acq_entry<double>(mu, var, noise, mask, values, best_val, best_idx, workspace, kind, best, xi, beta, sign, T, P, m,
                             idx_base, largest, first, strips, (hipStream_t)stream);
}

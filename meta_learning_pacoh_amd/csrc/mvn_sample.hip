// Joint draws from the (mixture) posterior predictive: y = y_mean + y_std (mu_c + L_c eps), L_c = chol(Sigma_c + j I).
// Replaces MultivariateNormal.rsample of the reference's predictive (AffineTransformedDistribution(likelihood(gp(x))),
// meta_learn/models.py:15-43, returned by GPR_meta_mll.py:181-186 / GPR_mll.py:194-198): gpytorch's psd_safe_cholesky of the
// covariance, then mean + L @ eps.
//
//   pacoh_mvn_factor: copy of the covariance (lower triangle mirrored, rung jitter on the diagonal) -> the dense Cholesky of
//                     dense.hip (dense_chol_launch: left-looking / MFMA right-looking / plain by size) on a zero residual, rung by
//                     rung for the problems that failed.  The input is never written.
//   pacoh_mvn_sample: Y = E L^T on the matrix cores (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64).  A workgroup owns 64 draws of
//                     ONE component x 64 output columns; the draws of the components follow each other in the grouped order, so the
//                     grid is proportional to the draws each component received.  L is staged in LDS slab by slab (lower triangle
//                     only: the slabs right of the diagonal are never visited), the eps rows are streamed from HBM into the MFMA A
//                     operand, and mu, the affine un-normalisation and the scatter back to draw order happen in the epilogue.
#include "common.h"

namespace pacoh {
namespace {

constexpr int SR = 64;                  // draws per workgroup (4 waves x 16)
constexpr int SC = 64;                  // output columns per workgroup (4 MFMA column tiles of 16)
constexpr int SK = 64;                  // k-slab width of the staged L tile
constexpr int SNT = 256;

template <typename T> struct SMf;
template <> struct SMf<float> {
    using acc = __attribute__((ext_vector_type(4))) float;
    static __device__ __forceinline__ acc mma(float a, float b, acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int lane, int r) { return 4 * (lane >> 4) + r; }      // C/D row of register r
};
template <> struct SMf<double> {
    using acc = __attribute__((ext_vector_type(4))) double;
    static __device__ __forceinline__ acc mma(double a, double b, acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }       // (f64: its own C/D map)
};

// L[b] = cov[b] (lower triangle mirrored) + jit I, for the problems still without a factor (attempt > 0: info[b] < 0)
template <typename T>
__global__ void __launch_bounds__(256) mvn_copy_jitter_kernel(const T* __restrict__ cov, T* __restrict__ L, const int32_t* __restrict__ info,
                                                              T jit, int attempt, int m) {
    const long b = blockIdx.x;
    if (attempt > 0 && info[b] >= 0) return;
    const int i = blockIdx.y;
    const T* C = cov + b * (long)m * m;
    T* row = L + (b * m + i) * (long)m;
    for (int j = threadIdx.x; j < m; j += 256)
        row[j] = j <= i ? C[(long)i * m + j] + (i == j ? jit : T(0)) : C[(long)j * m + i];
}

template <typename T>
__global__ void __launch_bounds__(SNT) mvn_sample_kernel(const T* __restrict__ L, const int32_t* __restrict__ info, const T* __restrict__ mu,
                                                         const T* __restrict__ eps, const int32_t* __restrict__ order,
                                                         const int32_t* __restrict__ offsets, T* __restrict__ out, T y_mean, T y_std,
                                                         int B, int m, int S, int vec_ok) {
    __shared__ T Ls[SC][SK + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.x;
    // ---- which component, and which 64 of its draws: a wave-wide scan over the components' tile counts -------------------------
    int c = 0, g0 = 0, cnt = S, rt = t;
    if (offsets) {
        int base = 0;
        bool found = false;
        for (int cb = 0; cb < B; cb += 64) {
            const int cc = cb + lane;
            const int o0 = cc < B ? offsets[cc] : 0, o1 = cc < B ? offsets[cc + 1] : 0;
            const int tiles = o1 > o0 ? (o1 - o0 + SR - 1) / SR : 0;
            int incl = tiles;
            for (int d = 1; d < 64; d <<= 1) {
                const int v = __shfl_up(incl, d, 64);
                if (lane >= d) incl += v;
            }
            const uint64_t hit = __ballot(base + incl > t);
            if (hit) {
                const int first = __ffsll((unsigned long long)hit) - 1;
                c = cb + first;
                rt = t - (base + __shfl(incl - tiles, first, 64));
                g0 = __shfl(o0, first, 64);
                cnt = __shfl(o1 - o0, first, 64);
                found = true;
                break;
            }
            base += __shfl(incl, 63, 64);
        }
        if (!found) return;                          // (the grid is sized for the worst case of the grouping)
    }
    const int r0 = rt * SR;
    if (r0 >= cnt) return;
    const int j0 = (gridDim.y - 1 - blockIdx.y) * SC;   // the long column tiles (most slabs) first
    const bool failed = info[c] < 0;
    const int q = lane >> 4, l15 = lane & 15;
    const int rw = r0 + 16 * wave;                   // first draw (within the component) of this wave
    const bool wave_live = rw < cnt;

    using Acc = typename SMf<T>::acc;
    Acc acc[4];
#pragma unroll
    for (int cs = 0; cs < 4; ++cs) acc[cs] = Acc{0, 0, 0, 0};
    if (!failed) {
        // A operand: lane (row l15, k-quarter q) holds eps[draw][k0 + 16 q + kk] for MFMA kk -- the k order inside a slab is permuted
        // alike for A and B, so every lane reads a contiguous run of 16 elements of its row
        const int ra = rw + l15;
        int da = -1;
        if (ra < cnt) {
            const int g = g0 + ra;
            da = order ? order[g] : g;
            if ((unsigned)da >= (unsigned)S) da = -1;
        }
        const T* erow = eps + (size_t)(da < 0 ? 0 : da) * m;
        const T* Lc = L + (size_t)c * m * m;
        const int kend = j0 + SC < m ? j0 + SC : m;
        for (int k0 = 0; k0 < kend; k0 += SK) {
            T a[16];
            const int kb = k0 + 16 * q;
            if (da >= 0 && vec_ok && kb + 16 <= m) {
                using V = typename VecOf<T>::type;
                constexpr int W = VecOf<T>::W;
                const V* p = reinterpret_cast<const V*>(erow + kb);
#pragma unroll
                for (int v = 0; v < 16 / W; ++v) {
                    const V x = p[v];
                    __builtin_memcpy(&a[v * W], &x, sizeof(V));
                }
            } else {
#pragma unroll
                for (int kk = 0; kk < 16; ++kk) a[kk] = (da >= 0 && kb + kk < m) ? erow[kb + kk] : T(0);
            }
            __syncthreads();                         // the previous slab has been consumed
            for (int e = tid; e < SC * SK; e += SNT) {
                const int i = e / SK, k = e - i * SK;
                const int gi = j0 + i, gk = k0 + k;
                Ls[i][k] = (gi < m && gk <= gi) ? Lc[(size_t)gi * m + gk] : T(0);   // (nothing above the diagonal is read)
            }
            __syncthreads();
            if (wave_live) {
#pragma unroll
                for (int kk = 0; kk < 16; ++kk)
#pragma unroll
                    for (int cs = 0; cs < 4; ++cs) acc[cs] = SMf<T>::mma(a[kk], Ls[16 * cs + l15][16 * q + kk], acc[cs]);
            }
        }
    }
    if (!wave_live) return;
    // ---- epilogue: mu, un-normalisation, scatter to draw order --------------------------------------------------------------------
    const T* muc = mu + (size_t)c * m;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int rr = rw + SMf<T>::row(lane, r);
        if (rr >= cnt) continue;
        const int g = g0 + rr;
        const int d = order ? order[g] : g;
        if ((unsigned)d >= (unsigned)S) continue;
        T* orow = out + (size_t)d * m;
#pragma unroll
        for (int cs = 0; cs < 4; ++cs) {
            const int col = j0 + 16 * cs + l15;
            if (col < m) orow[col] = failed ? T(NAN) : y_mean + y_std * (muc[col] + acc[cs][r]);
        }
    }
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

int dense_chol_launch(void* A, const void* resid, void* logp, void* alpha_out, int32_t* info, double scale, int B, int n,
                      int dtype, int attempt, hipStream_t stream, int u_only);                          // dense.hip
bool dense_chol_fits(int n, int dtype);                                                                  // dense.hip
}  // namespace pacoh

using namespace pacoh;

extern "C" size_t pacoh_mvn_factor_workspace_bytes(int B, int m, int dtype) {
    if ((dtype != PACOH_F32 && dtype != PACOH_F64) || B <= 0 || m <= 0) return 0;
    const size_t es = dtype == PACOH_F64 ? 8 : 4;
    return align256((size_t)B * m * es) + align256((size_t)B * es);       // zero residual [B,m] | log-density [B]
}

extern "C" int pacoh_mvn_factor(const void* cov, void* L, int32_t* info, void* workspace, int B, int m, int dtype, void* stream) {
    if (check_dtype(dtype)) return PACOH_EDTYPE;
    if (!cov || !L || !info || !workspace || B <= 0 || m <= 0) return PACOH_EINVAL;
    if (m > 65535 || !dense_chol_fits(m, dtype)) return PACOH_ELIMIT;      // (before anything is enqueued)
    hipStream_t s = (hipStream_t)stream;
    const size_t es = dtype == PACOH_F64 ? 8 : 4;
    void* resid = workspace;
    void* logp = (unsigned char*)workspace + align256((size_t)B * m * es);
    if (hipMemsetAsync(resid, 0, (size_t)B * m * es, s) != hipSuccess) { (void)hipGetLastError(); return PACOH_ELAUNCH; }
    const double jitter_base = dtype == PACOH_F32 ? 1e-6 : 1e-8;            // psd_safe_cholesky [gpytorch-upstream], as dense_gp.hip
    // all four rungs are enqueued without reading info back (no host sync; graph-capturable): rungs 1..3 are a copy launch and a
    // factorisation launch each whose workgroups exit at once for the components that already have a factor
    for (int attempt = 0; attempt < 4; ++attempt) {
        double jit = 0.0;
        if (attempt > 0) {
            jit = jitter_base;
            for (int k = 1; k < attempt; ++k) jit *= 10.0;
        }
        if (dtype == PACOH_F32)
            hipLaunchKernelGGL(mvn_copy_jitter_kernel<float>, dim3(B, m), dim3(256), 0, s, (const float*)cov, (float*)L, (const int32_t*)info,
                               (float)jit, attempt, m);
        else
            hipLaunchKernelGGL(mvn_copy_jitter_kernel<double>, dim3(B, m), dim3(256), 0, s, (const double*)cov, (double*)L, (const int32_t*)info,
                               jit, attempt, m);
        int rc = launch_status();
        if (rc) return rc;
        rc = dense_chol_launch(L, resid, logp, nullptr, info, 1.0, B, m, dtype, attempt, s, 0);
        if (rc) return rc;
    }
    return PACOH_OK;
}

extern "C" int pacoh_mvn_sample(const void* L, const int32_t* info, const void* mu, const void* eps, const int32_t* order,
                                const int32_t* offsets, void* out, double y_mean, double y_std, int B, int m, int S, int dtype,
                                void* stream) {
    if (check_dtype(dtype)) return PACOH_EDTYPE;
    if (!L || !info || !mu || !eps || !out || B <= 0 || m <= 0 || S < 0) return PACOH_EINVAL;
    if ((order == nullptr) != (offsets == nullptr) || (B > 1 && !offsets)) return PACOH_EINVAL;
    if (S == 0) return PACOH_OK;
    const long tiles = ((long)S + SR - 1) / SR + (offsets ? (B < S ? B : S) : 0);   // sum_c ceil(n_c / 64) <= this
    const long ctiles = ((long)m + SC - 1) / SC;
    if (tiles > 0x7fffffffL || ctiles > 65535) return PACOH_ELIMIT;
    const int es = dtype == PACOH_F64 ? 8 : 4;
    const int vec_ok = (m % (16 / es) == 0) && ((uintptr_t)eps % 16 == 0);
    const dim3 grid((unsigned)tiles, (unsigned)ctiles);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PACOH_F32)
        hipLaunchKernelGGL(mvn_sample_kernel<float>, grid, dim3(SNT), 0, s, (const float*)L, info, (const float*)mu, (const float*)eps, order,
                           offsets, (float*)out, (float)y_mean, (float)y_std, B, m, S, vec_ok);
    else
        hipLaunchKernelGGL(mvn_sample_kernel<double>, grid, dim3(SNT), 0, s, (const double*)L, info, (const double*)mu, (const double*)eps,
                           order, offsets, (double*)out, y_mean, y_std, B, m, S, vec_ok);
    return launch_status();
}

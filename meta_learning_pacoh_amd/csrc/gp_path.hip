// Pathwise posterior function draws on the conditioned GP (Matheron's rule on a random-Fourier-feature prior; Wilson et al. 2020,
// "Efficiently sampling functions from Gaussian process posteriors").  With u = z / lengthscale, the state (zs, resid, X, info) of
// gp_cond.hip, j the jitter of the rung in info, D features phi_d(u) = sqrt(2 os / D) cos(omega_d . u + phase_d) and S draws
// (w_s [D], eps_s [n]) per problem:
//   pacoh_gp_path_fit   v_s = (K + j I)^-1 (resid - Phi(zs) w_s - sqrt(noise + j) eps_s) = X^T X (...).  One workgroup per (problem,
//                       16 draws), a thread per context point: the feature sums in registers (omega / phase / w staged in LDS by
//                       64 columns), then U = X R and v = X^T U with X staged slab by slab in LDS, at or below the diagonal and
//                       below row n only.  Plain FMA: it runs once per set of draws.
//   pacoh_gp_path_eval  f_s(x*) = m(x*) + sum_d phi_d(u*) w_sd + sum_i os k(u*, u_i) v_si: ONE GEMM [m x (D + n)] . [(D + n) x S] on
//                       the matrix cores (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64) whose left operand is never stored.
//                       Grid = problems x tiles of 64 test points x groups of up to 64 draws; four waves of 16 test points.  The
//                       K loop runs over 16-wide slabs of the D + n columns (D % 16 == 0: a slab is all features or all context
//                       points), staged 64 columns at a time: A in registers (features from omega / phase, then kernel columns from
//                       zs via kern_val), each value computed ONCE per workgroup and used for all of its draw tiles; B from w / v in
//                       LDS.  The cosine is the library's (full-range argument reduction): Matern-1/2 frequencies are Cauchy-tailed
//                       and arguments of 1e3 .. 1e5 radians occur.
//   pacoh_gp_path_argmax  per draw, the eligible test point with the greatest / smallest f_s: the SAME K loop (path_tile(), one device
//                       function for both kernels, so the values compared are the eval kernel's bit for bit), a strip of test tiles
//                       per workgroup, a wave-level (value, first index) reduction per draw instead of the stores, one partial pair
//                       per (problem, draw, strip), and a second small launch that merges strips and the caller's running best.
// CMf / rung_jitter are DUPLICATED from gp_cond.hip, which stays as it is.
#include "common.h"

namespace pacoh {
namespace {

template <typename T> struct CMf;
template <> struct CMf<float> {
    using acc = __attribute__((ext_vector_type(4))) float;
    static constexpr int MAXT = 12;     // 16-point tiles of the context: 192 >= the fp32 limit
    static __device__ __forceinline__ acc mma(float a, float b, acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int lane, int r) { return 4 * (lane >> 4) + r; }
};
template <> struct CMf<double> {
    using acc = __attribute__((ext_vector_type(4))) double;
    static constexpr int MAXT = 9;      // 144 >= the fp64 limit
    static __device__ __forceinline__ acc mma(double a, double b, acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }
};

// jitter of ladder rung r (0: none), multiplied up in T exactly as the ladder does
template <typename T> __device__ __forceinline__ T rung_jitter(int rung) {
    if (rung <= 0) return T(0);
    T j = sizeof(T) == 4 ? T(1e-6) : T(1e-8);
    for (int q = 1; q < rung; ++q) j *= T(10);
    return j;
}

template <typename T> __device__ __forceinline__ T t_cos(T x);
template <> __device__ __forceinline__ float t_cos<float>(float x) { return cosf(x); }
template <> __device__ __forceinline__ double t_cos<double>(double x) { return cos(x); }

// one random feature at the scaled point u: amp cos(omega . u + phase), the sum in the order c = 0 .. FP-1 (padded entries are 0)
template <typename T, int FP>
__device__ __forceinline__ T rff_val(const T* __restrict__ om, T ph, const T (&u)[FP], T amp) {
    T arg = ph;
#pragma unroll
    for (int c = 0; c < FP; ++c) arg = fma(om[c], u[c], arg);
    return amp * t_cos<T>(arg);
}

constexpr int PK = 64;                  // columns of the D + n staged at a time (4 MFMA slabs of 16)
constexpr int PKP = PK + 4;             // LDS row stride: 4 x odd words, so a lane's four k entries are one aligned 16 / 32 byte read

// ======================================================================================================================== fit
constexpr int FS = 16;                  // draws per workgroup
constexpr int FNT = 256;                // threads: one per context point (>= the largest capacity, checked by the launcher)

template <typename T>
struct PathFitArgs {
    const T* zs; const T* resid; const T* X; const int32_t* info;
    const T* os; const T* noise; const T* omega; const T* phase; const T* w; const T* eps;
    T* v;
    int B, P, n, cap, S, D, f, groups;
};

template <typename T, int FP>
__global__ void __launch_bounds__(FNT) gp_path_fit_kernel(PathFitArgs<T> a) {
    constexpr int MAXR = CMf<T>::MAXT * 16;
    __shared__ T wL[FS][PK + 1];
    __shared__ T omL[PK * FP];
    __shared__ T phL[PK];
    __shared__ T RL[FS][MAXR];           // R, later U: [draw][context point]
    __shared__ T XsL[MAXR * 17];         // a slab of X: 16 columns of all rows [MAXR][17], later 16 rows of all columns [16][MAXR + 1]
    const int tid = threadIdx.x;
    const int grp = (int)(blockIdx.x % (unsigned)a.groups);
    const long b = blockIdx.x / (unsigned)a.groups;
    const int p = (int)(b % a.P);
    const int n = a.n, cap = a.cap, f = a.f, S = a.S, D = a.D;
    const int s_base = grp * FS;
    const int ns = min(FS, S - s_base);
    const int rung = a.info[b];
    T* vg = a.v + (b * S + s_base) * (long)n;
    if (rung < 0) {                                  // (uniform per workgroup)
        for (int e = tid; e < ns * n; e += FNT) vg[e] = T(NAN);
        return;
    }
    const int i = tid;
    const bool live = i < n;
    const T os = a.os ? a.os[p] : T(1);
    const T amp = t_sqrt<T>(T(2) * os / T(D));
    T zi[FP];
#pragma unroll
    for (int c = 0; c < FP; ++c) zi[c] = (live && c < f) ? a.zs[(b * cap + i) * (long)f + c] : T(0);
    const T* wg = a.w + (b * S + s_base) * (long)D;

    // ---- Phi(zs) w: the features of this thread's point, 64 columns of omega / phase / w in LDS at a time ----------------------------
    T acc[FS];
#pragma unroll
    for (int s = 0; s < FS; ++s) acc[s] = 0;
    for (int c0 = 0; c0 < D; c0 += PK) {
        const int kcN = min(PK, D - c0);
        __syncthreads();                             // the previous chunk has been consumed
        for (int e = tid; e < FS * PK; e += FNT) {
            const int s = e / PK, kc = e - s * PK;
            wL[s][kc] = (s < ns && kc < kcN) ? wg[(long)s * D + c0 + kc] : T(0);
        }
        for (int e = tid; e < PK * FP; e += FNT) {
            const int kc = e / FP, c = e - kc * FP;
            omL[e] = (kc < kcN && c < f) ? a.omega[(long)(c0 + kc) * f + c] : T(0);
        }
        if (tid < PK) phL[tid] = tid < kcN ? a.phase[c0 + tid] : T(0);
        __syncthreads();
        if (live) {
            for (int kc = 0; kc < kcN; ++kc) {
                const T phi = rff_val<T, FP>(omL + kc * FP, phL[kc], zi, amp);
#pragma unroll
                for (int s = 0; s < FS; ++s) acc[s] = fma(phi, wL[s][kc], acc[s]);
            }
        }
    }
    // ---- R = resid - Phi w - sqrt(noise + j) eps -------------------------------------------------------------------------------------
    if (live) {
        const T sj = t_sqrt<T>(a.noise[p] + rung_jitter<T>(rung));
        const T ri = a.resid[b * cap + i];
        const T* eg = a.eps + (b * S + s_base) * (long)n + i;
#pragma unroll
        for (int s = 0; s < FS; ++s) RL[s][i] = s < ns ? ri - acc[s] - sj * eg[(long)s * n] : T(0);
    }
    const T* Xg = a.X + b * (long)cap * cap;
    const int NT = (n + 15) >> 4;
    // ---- U = X R: 16 columns of X (rows k0 .. n-1, at or below the diagonal) per slab; thread i owns row i ---------------------------
#pragma unroll
    for (int s = 0; s < FS; ++s) acc[s] = 0;
    for (int kt = 0; kt < NT; ++kt) {
        const int k0 = kt * 16;
        __syncthreads();                             // R complete (first slab); the previous slab has been consumed
        for (int e = tid; e < (n - k0) * 16; e += FNT) {
            const int r = k0 + (e >> 4), kc = e & 15;
            XsL[r * 17 + kc] = (k0 + kc <= r) ? Xg[(long)r * cap + k0 + kc] : T(0);
        }
        __syncthreads();
        if (live && i >= k0) {
            const int kcN = min(16, i - k0 + 1);     // columns k0 .. min(k0 + 15, i): nothing above the diagonal
            for (int kc = 0; kc < kcN; ++kc) {
                const T x = XsL[i * 17 + kc];
#pragma unroll
                for (int s = 0; s < FS; ++s) acc[s] = fma(x, RL[s][k0 + kc], acc[s]);
            }
        }
    }
    __syncthreads();                                 // every thread has read R
    if (live) {
#pragma unroll
        for (int s = 0; s < FS; ++s) RL[s][i] = acc[s];
    }
    // ---- v = X^T U: 16 rows of X (columns 0 .. row) per slab; thread k owns column k -------------------------------------------------
#pragma unroll
    for (int s = 0; s < FS; ++s) acc[s] = 0;
    for (int it = 0; it < NT; ++it) {
        const int i0 = it * 16;
        const int rows = min(16, n - i0);
        __syncthreads();                             // U complete (first slab); the previous slab has been consumed
        for (int e = tid; e < rows * n; e += FNT) {
            const int rl = e / n, k = e - rl * n, r = i0 + rl;
            XsL[rl * (MAXR + 1) + k] = (k <= r) ? Xg[(long)r * cap + k] : T(0);
        }
        __syncthreads();
        if (live) {
            for (int rl = max(0, i - i0); rl < rows; ++rl) {     // rows r >= k only
                const T x = XsL[rl * (MAXR + 1) + i];
#pragma unroll
                for (int s = 0; s < FS; ++s) acc[s] = fma(x, RL[s][i0 + rl], acc[s]);
            }
        }
    }
    if (live) {
#pragma unroll
        for (int s = 0; s < FS; ++s) if (s < ns) vg[(long)s * n + i] = acc[s];
    }
}

// ======================================================================================================================= eval
constexpr int PT = 64;                  // test points per workgroup (4 waves x 16)
constexpr int PS = 64;                  // draws per workgroup (up to 4 accumulator tiles of 16 per wave)
constexpr int PNT = 256;

template <typename T>
struct PathEvalArgs {
    const T* zs; const T* v; const T* w; const int32_t* info; const T* omega; const T* phase;
    const T* z_tst; int zt_div; const T* mean_tst; int mean_mode; const T* ls; const T* os;
    T* out;
    int B, P, n, cap, S, D, m, f, kind, tiles, groups;
};

// The K loop of one tile of 64 test points x up to 64 draws, shared by both epilogues (ONE piece of device code: the values the argmax
// epilogue compares are the values the eval epilogue stores, bit for bit).  On return Bs holds the tile [draw][test point] WITHOUT
// the mean, behind a barrier.  zsL is staged by the caller; the first barrier in here covers it.
template <typename T, int FP>
__device__ __forceinline__ void path_tile(const PathEvalArgs<T>& a, long b, int p, int t0, int s_base, int ns, int NDT,
                                          T (&Bs)[PS][PKP], T* __restrict__ omL, T* __restrict__ phL, const T* __restrict__ zsL) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4, l15 = lane & 15;
    const int n = a.n, m = a.m, f = a.f, S = a.S, D = a.D;
    // the A operand's row of this lane: test point ta, features divided by the lengthscales as gp_cond.hip does
    const int ta = t0 + 16 * wave + l15;
    const T os = a.os ? a.os[p] : T(1);
    const T amp = t_sqrt<T>(T(2) * os / T(D));
    T zt[FP];
#pragma unroll
    for (int c = 0; c < FP; ++c) zt[c] = 0;
    if (ta < m) {
        const T* zp = a.z_tst + ((b / a.zt_div) * m + ta) * (long)f;
#pragma unroll
        for (int c = 0; c < FP; ++c) if (c < f) zt[c] = zp[c] / a.ls[(long)p * f + c];
    }
    const bool wave_live = t0 + 16 * wave < m;
    using Acc = typename CMf<T>::acc;
    Acc acc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc[dt] = Acc{0, 0, 0, 0};
    const int NT = (n + 15) >> 4;
    const int Ctot = D + 16 * NT;                    // columns: D features, then the context points padded to whole slabs
    const T* wg = a.w + (b * S + s_base) * (long)D;
    const T* vg = a.v + (b * S + s_base) * (long)n;

    for (int c0 = 0; c0 < Ctot; c0 += PK) {
        const int kcN = min(PK, Ctot - c0);          // a multiple of 16
        __syncthreads();                             // zsL staged (first chunk); the previous chunk / tile has been consumed
        for (int e = tid; e < NDT * 16 * PK; e += PNT) {
            const int s = e >> 6, kc = e & 63, col = c0 + kc;
            T val = 0;
            if (s < ns && kc < kcN) {
                if (col < D) val = wg[(long)s * D + col];
                else if (col - D < n) val = vg[(long)s * n + (col - D)];
            }
            Bs[s][kc] = val;
        }
        if (c0 < D) {
            for (int e = tid; e < PK * FP; e += PNT) {
                const int kc = e / FP, c = e - kc * FP, col = c0 + kc;
                omL[e] = (col < D && c < f) ? a.omega[(long)col * f + c] : T(0);
            }
            if (tid < PK) phL[tid] = c0 + tid < D ? a.phase[c0 + tid] : T(0);
        }
        __syncthreads();
        for (int sl = 0; sl < (kcN >> 4); ++sl) {
            const int k0 = c0 + 16 * sl;             // the slab: all features (k0 < D) or all context points (uniform)
            // A[ta, k0 + 4 q + kk], kk = 0..3: MFMA step kk contracts the four columns {k0 + 4 q + kk : q = 0..3} -- the k order inside
            // a slab is permuted alike for A and B
            T av[4];
            if (k0 < D) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int kc = 16 * sl + 4 * q + kk;
                    av[kk] = rff_val<T, FP>(omL + kc * FP, phL[kc], zt, amp);
                }
            } else {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int j = k0 - D + 4 * q + kk;           // < 16 NT <= MAXR
                    T s2 = 0;
#pragma unroll
                    for (int c = 0; c < FP; ++c) { T d = zt[c] - zsL[j * FP + c]; s2 = fma(d, d, s2); }
                    av[kk] = j < n ? os * kern_val<T>(a.kind, s2) : T(0);
                }
            }
            if (wave_live) {
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    if (dt < NDT) {                  // (uniform)
                        const T* bp = &Bs[16 * dt + l15][16 * sl + 4 * q];
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) acc[dt] = CMf<T>::mma(av[kk], bp[kk], acc[dt]);
                    }
                }
            }
        }
    }
    // ---- the output tile through LDS: [draw][test point], so that a draw's 64 test points are one contiguous row --------------------
    __syncthreads();
    if (wave_live) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            if (dt < NDT) {
#pragma unroll
                for (int r = 0; r < 4; ++r) Bs[16 * dt + l15][16 * wave + CMf<T>::row(lane, r)] = acc[dt][r];
            }
        }
    }
    __syncthreads();
}

// the prior mean of test point t (global index in [0, m)) of problem b
template <typename T>
__device__ __forceinline__ T path_mean(const PathEvalArgs<T>& a, long b, int p, int t) {
    T mt = 0;
    if (a.mean_mode == PACOH_MEAN_VECTOR) mt = a.mean_tst[b * a.m + t];
    else if (a.mean_mode == PACOH_MEAN_CONST) mt = a.mean_tst[p];
    return mt;
}

template <typename T, int FP>
__device__ __forceinline__ void path_stage_zs(const PathEvalArgs<T>& a, long b, T* __restrict__ zsL) {
    constexpr int MAXR = CMf<T>::MAXT * 16;
    const T* zsg = a.zs + b * (long)a.cap * a.f;
    for (int e = threadIdx.x; e < MAXR * FP; e += PNT) {
        const int j = e / FP, c = e - j * FP;
        zsL[e] = (j < a.n && c < a.f) ? zsg[(long)j * a.f + c] : T(0);
    }
}

template <typename T, int FP>
__global__ void __launch_bounds__(PNT) gp_path_eval_kernel(PathEvalArgs<T> a) {
    constexpr int MAXR = CMf<T>::MAXT * 16;
    __shared__ __attribute__((aligned(32))) T Bs[PS][PKP];       // [draw][column of the chunk]; the output tile [draw][test point] at the end
    __shared__ T omL[PK * FP];
    __shared__ T phL[PK];
    __shared__ T zsL[MAXR * FP];
    const int tid = threadIdx.x;
    const int grp = (int)(blockIdx.x % (unsigned)a.groups);
    const unsigned bt = blockIdx.x / (unsigned)a.groups;
    const int tile = (int)(bt % (unsigned)a.tiles);
    const long b = bt / (unsigned)a.tiles;
    const int p = (int)(b % a.P);
    const int m = a.m, S = a.S;
    const int t0 = tile * PT, s_base = grp * PS;
    const int ns = min(PS, S - s_base);              // draws of this workgroup
    const int NDT = (ns + 15) >> 4;                  // their 16-wide tiles (uniform)
    T* og = a.out + (b * S + s_base) * (long)m + t0;

    if (a.info[b] < 0) {                             // (uniform per workgroup)
        for (int e = tid; e < PS * PT; e += PNT) {
            const int s = e >> 6, t = e & 63;
            if (s < ns && t0 + t < m) og[(long)s * m + t] = T(NAN);
        }
        return;
    }
    path_stage_zs<T, FP>(a, b, zsL);
    path_tile<T, FP>(a, b, p, t0, s_base, ns, NDT, Bs, omL, phL, zsL);
    for (int e = tid; e < NDT * 16 * PT; e += PNT) {
        const int s = e >> 6, t = e & 63;
        if (s < ns && t0 + t < m) og[(long)s * m + t] = path_mean<T>(a, b, p, t0 + t) + Bs[s][t];
    }
}

// ===================================================================================================================== argmax
// Per (problem, draw): the eligible test point with the greatest (largest = 1) or smallest value of the eval kernel, ties (==) to the
// smaller global index idx_base + t, NaN never wins, nothing eligible: idx -1 / val NaN.  A workgroup takes a STRIP of consecutive
// test tiles of one (problem, group of draws): per tile the K loop above, then wave w reduces the rows w, w + 4, ... of the tile in
// LDS (a lane per test point: the extremum by six xor-shuffles, the first lane that holds it by a ballot) and lane k of the wave
// keeps the running pair of row w + 4 k.  Tiles ascend inside a strip, so a later tile wins only when strictly better.  One partial
// pair per (problem, draw, strip) goes to the workspace; gp_path_argmax_merge_kernel (a wave per (problem, draw)) merges the strips
// and, with first = 0, the pair already in best_val / best_idx by (value, smaller index).  No atomics, no waiting: deterministic.
template <typename T>
struct PathArgmaxArgs {
    PathEvalArgs<T> e;                  // out unused
    const uint8_t* mask;
    int64_t* part_idx; T* part_val;     // [B][S][strips]
    T* best_val; int64_t* best_idx;     // [B][S]
    int64_t idx_base;
    int strips, largest, first;
};

template <typename T> __device__ __forceinline__ T shfl_xor_t(T x, int d);
template <> __device__ __forceinline__ float shfl_xor_t<float>(float x, int d) { return __shfl_xor(x, d, 64); }
template <> __device__ __forceinline__ double shfl_xor_t<double>(double x, int d) { return __shfl_xor(x, d, 64); }
template <typename T> __device__ __forceinline__ T shfl_t(T x, int src);
template <> __device__ __forceinline__ float shfl_t<float>(float x, int src) { return __shfl(x, src, 64); }
template <> __device__ __forceinline__ double shfl_t<double>(double x, int src) { return __shfl(x, src, 64); }

// is the pair (vb, ib) ahead of (va, ia)?  idx < 0 marks "nothing"; values of pairs with idx >= 0 are never NaN
template <typename T>
__device__ __forceinline__ bool pair_ahead(T va, int64_t ia, T vb, int64_t ib, int largest) {
    if (ib < 0) return false;
    if (ia < 0) return true;
    if (vb == va) return ib < ia;
    return largest ? vb > va : vb < va;
}

// FP <= 4 is asked for the eval kernel's five (fp32) / three (fp64) waves per SIMD: the running pairs cost about ten registers, one
// wave without the request; with it the accumulators stay in VGPRs and nothing spills (profiles/path_argmax_kernel_resources.txt)
template <typename T, int FP>
__global__ void __launch_bounds__(PNT) __attribute__((amdgpu_waves_per_eu(FP <= 4 ? (sizeof(T) == 4 ? 5 : 3) : 1, 8)))
gp_path_argmax_kernel(PathArgmaxArgs<T> g) {
    constexpr int MAXR = CMf<T>::MAXT * 16;
    __shared__ __attribute__((aligned(32))) T Bs[PS][PKP];
    __shared__ T omL[PK * FP];
    __shared__ T phL[PK];
    __shared__ T zsL[MAXR * FP];
    const PathEvalArgs<T>& a = g.e;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = (int)(blockIdx.x % (unsigned)a.groups);
    const unsigned bt = blockIdx.x / (unsigned)a.groups;
    const int strip = (int)(bt % (unsigned)g.strips);
    const long b = bt / (unsigned)g.strips;
    const int p = (int)(b % a.P);
    const int m = a.m, S = a.S;
    const int s_base = grp * PS;
    const int ns = min(PS, S - s_base);
    const int NDT = (ns + 15) >> 4;
    const int tile_lo = (int)((long)strip * a.tiles / g.strips), tile_hi = (int)((long)(strip + 1) * a.tiles / g.strips);
    // lane k < 16 of wave w: the running pair of draw s_base + w + 4 k (tile-local index of the point inside [0, m))
    T run_v = T(NAN);
    int run_t = -1;
    if (a.info[b] >= 0) {                            // (uniform per workgroup)
        path_stage_zs<T, FP>(a, b, zsL);
        const T lose = g.largest ? -T(INFINITY) : T(INFINITY);
        for (int tile = tile_lo; tile < tile_hi; ++tile) {
            const int t0 = tile * PT;
            path_tile<T, FP>(a, b, p, t0, s_base, ns, NDT, Bs, omL, phL, zsL);
            const int t = t0 + lane;
            const bool in = t < m && (!g.mask || g.mask[t] != 0);
            const T mt = t < m ? path_mean<T>(a, b, p, t) : T(0);
            for (int k = 0; 4 * k + wave < ns; ++k) {            // (uniform per wave)
                const T fv = mt + Bs[4 * k + wave][lane];
                const bool ok = in && fv == fv;
                T ext = ok ? fv : lose;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    const T o = shfl_xor_t<T>(ext, d);
                    ext = g.largest ? (o > ext ? o : ext) : (o < ext ? o : ext);
                }
                const unsigned long long hit = __ballot(ok && fv == ext);
                if (hit) {                                       // (uniform per wave)
                    const int win = __ffsll((long long)hit) - 1;
                    const T wv = shfl_t<T>(fv, win);             // the winner's own bits: -0.0 and +0.0 tie
                    if (lane == k && (run_t < 0 || (g.largest ? wv > run_v : wv < run_v))) { run_v = wv; run_t = t0 + win; }
                }
            }
        }
    }
    if (lane < 16 && 4 * lane + wave < ns) {
        const long o = ((b * S + s_base + 4 * lane + wave) * (long)g.strips) + strip;
        g.part_val[o] = run_v;
        g.part_idx[o] = run_t < 0 ? (int64_t)-1 : g.idx_base + run_t;
    }
}

template <typename T>
__global__ void __launch_bounds__(PNT) gp_path_argmax_merge_kernel(PathArgmaxArgs<T> g) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (PNT / 64) + (threadIdx.x >> 6);         // (problem, draw)
    const long rows = (long)g.e.B * g.e.S;
    if (row >= rows) return;                         // (uniform per wave)
    T bv = T(NAN);
    int64_t bi = -1;
    if (g.e.info[row / g.e.S] >= 0) {
        for (int st = lane; st < g.strips; st += 64) {
            const T v = g.part_val[row * g.strips + st];
            const int64_t i = g.part_idx[row * g.strips + st];
            if (pair_ahead<T>(bv, bi, v, i, g.largest)) { bv = v; bi = i; }
        }
        if (lane == 0 && !g.first) {
            const T v = g.best_val[row];
            const int64_t i = v == v ? g.best_idx[row] : (int64_t)-1;
            if (pair_ahead<T>(bv, bi, v, i, g.largest)) { bv = v; bi = i; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const T v = shfl_xor_t<T>(bv, d);
            const int lo = __shfl_xor((int)(bi & 0xffffffffLL), d, 64), hi = __shfl_xor((int)(bi >> 32), d, 64);
            const int64_t i = ((int64_t)hi << 32) | (uint32_t)lo;
            if (pair_ahead<T>(bv, bi, v, i, g.largest)) { bv = v; bi = i; }
        }
    }
    if (lane == 0) {
        g.best_val[row] = bi < 0 ? T(NAN) : bv;
        g.best_idx[row] = bi;
    }
}

inline int fp_of(int f) { return f <= 2 ? 2 : (f <= 4 ? 4 : (f <= 8 ? 8 : 16)); }

// the checks the two entry points share (after the dtype): 0, or the error code
int path_common(int B, int P, int n, int cap, int S, int D, int f_arg, int dtype) {
    if (B <= 0 || P <= 0 || features_of(f_arg) <= 0) return PACOH_EINVAL;
    const int kind = kernel_of(f_arg);
    if (features_of(f_arg) > PACOH_MAX_FEATURES || !family_known(kind)) return PACOH_ELIMIT;
    if (kind == PACOH_KERNEL_COSINE) return PACOH_ELIMIT;        // no spectral density of this form for f > 1
    const int maxr = (dtype == PACOH_F32 ? CMf<float>::MAXT : CMf<double>::MAXT) * 16;
    if (n < 1 || n > cap || cap > pacoh_gp_cond_max_n(dtype) || cap > maxr || cap > FNT) return PACOH_ELIMIT;
    if (S < 1 || D < 16 || D > 16384 || (D % 16) != 0) return PACOH_ELIMIT;
    return PACOH_OK;
}

template <typename T>
int path_fit_entry(const void* zs, const void* resid, const void* X, const int32_t* info, const void* os, const void* noise,
                   const void* omega, const void* phase, const void* w, const void* eps, void* v,
                   int B, int P, int n, int cap, int S, int D, int f, hipStream_t stream) {
    PathFitArgs<T> a = {};
    a.zs = (const T*)zs; a.resid = (const T*)resid; a.X = (const T*)X; a.info = info; a.os = (const T*)os; a.noise = (const T*)noise;
    a.omega = (const T*)omega; a.phase = (const T*)phase; a.w = (const T*)w; a.eps = (const T*)eps; a.v = (T*)v;
    a.B = B; a.P = P; a.n = n; a.cap = cap; a.S = S; a.D = D; a.f = features_of(f);
    a.groups = (S + FS - 1) / FS;
    const long blocks = (long)a.groups * B;
    if (blocks > 0x7fffffffL) return PACOH_ELIMIT;
    void (*kern)(PathFitArgs<T>) = nullptr;
    switch (fp_of(a.f)) {
        case 2: kern = gp_path_fit_kernel<T, 2>; break;
        case 4: kern = gp_path_fit_kernel<T, 4>; break;
        case 8: kern = gp_path_fit_kernel<T, 8>; break;
        default: kern = gp_path_fit_kernel<T, 16>; break;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(FNT), 0, stream, a);
    return launch_status();
}

template <typename T>
int path_eval_entry(const void* zs, const void* v, const void* w, const int32_t* info, const void* omega, const void* phase,
                    const void* z_tst, int zt_div, const void* mean_tst, int mean_mode, const void* ls, const void* os, void* out,
                    int B, int P, int n, int cap, int S, int D, int m, int f, hipStream_t stream) {
    PathEvalArgs<T> a = {};
    a.zs = (const T*)zs; a.v = (const T*)v; a.w = (const T*)w; a.info = info; a.omega = (const T*)omega; a.phase = (const T*)phase;
    a.z_tst = (const T*)z_tst; a.zt_div = zt_div; a.mean_tst = (const T*)mean_tst; a.mean_mode = mean_mode;
    a.ls = (const T*)ls; a.os = (const T*)os; a.out = (T*)out;
    a.B = B; a.P = P; a.n = n; a.cap = cap; a.S = S; a.D = D; a.m = m; a.f = features_of(f); a.kind = kernel_of(f);
    a.tiles = (m + PT - 1) / PT;
    a.groups = (S + PS - 1) / PS;
    const long bt = (long)a.tiles * B;
    if (bt > 0x7fffffffL || bt * a.groups > 0x7fffffffL) return PACOH_ELIMIT;
    void (*kern)(PathEvalArgs<T>) = nullptr;
    switch (fp_of(a.f)) {
        case 2: kern = gp_path_eval_kernel<T, 2>; break;
        case 4: kern = gp_path_eval_kernel<T, 4>; break;
        case 8: kern = gp_path_eval_kernel<T, 8>; break;
        default: kern = gp_path_eval_kernel<T, 16>; break;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)(bt * a.groups)), dim3(PNT), 0, stream, a);
    return launch_status();
}

// workgroups per group of draws that strips = 0 aims at.  Measured on the MI355X: the launch is fastest with one tile per
// strip and loses 5 - 10 % at 16 workgroups per CU (strips of 7 - 8 tiles leave the last round uneven), so the bound is there to cap
// the partials of a very large call (12 bytes per pair: 6 MB at S = 16), not to make strips long
constexpr long ARGMAX_GRID = 32768;

// strips of a call: a positive request clamped to the tile count; 0: ARGMAX_GRID / B, at least 1, at most the tile count
inline int argmax_strips(int B, int m, int strips) {
    const long tiles = ((long)m + PT - 1) / PT;
    const long want = strips > 0 ? strips : (ARGMAX_GRID + B - 1) / B;
    return (int)std::max(1L, std::min(want, tiles));
}

// partial pairs the workspace holds: the call's own B S strips for a positive request; for strips = 0 the bound
// S min(B tiles, ARGMAX_GRID - 1 + B) >= B S strips, which unlike the exact count never shrinks as B or S grow
inline size_t argmax_pairs(int B, int S, int m, int strips) {
    const long tiles = ((long)m + PT - 1) / PT;
    if (strips > 0) return (size_t)B * S * (size_t)argmax_strips(B, m, strips);
    return (size_t)S * (size_t)std::min((long)B * tiles, ARGMAX_GRID - 1 + B);
}

template <typename T>
int path_argmax_entry(const void* zs, const void* v, const void* w, const int32_t* info, const void* omega, const void* phase,
                      const void* z_tst, int zt_div, const void* mean_tst, int mean_mode, const void* ls, const void* os,
                      const uint8_t* mask, void* best_val, int64_t* best_idx, void* workspace,
                      int B, int P, int n, int cap, int S, int D, int m, int f, int64_t idx_base, int largest, int first, int strips,
                      hipStream_t stream) {
    PathArgmaxArgs<T> g = {};
    PathEvalArgs<T>& a = g.e;
    a.zs = (const T*)zs; a.v = (const T*)v; a.w = (const T*)w; a.info = info; a.omega = (const T*)omega; a.phase = (const T*)phase;
    a.z_tst = (const T*)z_tst; a.zt_div = zt_div; a.mean_tst = (const T*)mean_tst; a.mean_mode = mean_mode;
    a.ls = (const T*)ls; a.os = (const T*)os; a.out = nullptr;
    a.B = B; a.P = P; a.n = n; a.cap = cap; a.S = S; a.D = D; a.m = m; a.f = features_of(f); a.kind = kernel_of(f);
    a.tiles = (m + PT - 1) / PT;
    a.groups = (S + PS - 1) / PS;
    g.strips = argmax_strips(B, m, strips);
    g.mask = mask; g.best_val = (T*)best_val; g.best_idx = best_idx; g.idx_base = idx_base; g.largest = largest; g.first = first;
    const long pairs = (long)B * S * g.strips;
    g.part_idx = (int64_t*)workspace;                // the 8-byte entries first: both arrays stay aligned
    g.part_val = (T*)(g.part_idx + pairs);
    const long bs = (long)g.strips * B;
    const long rows = ((long)B * S + PNT / 64 - 1) / (PNT / 64);
    if (bs > 0x7fffffffL || bs * a.groups > 0x7fffffffL || rows > 0x7fffffffL) return PACOH_ELIMIT;
    void (*kern)(PathArgmaxArgs<T>) = nullptr;
    switch (fp_of(a.f)) {
        case 2: kern = gp_path_argmax_kernel<T, 2>; break;
        case 4: kern = gp_path_argmax_kernel<T, 4>; break;
        case 8: kern = gp_path_argmax_kernel<T, 8>; break;
        default: kern = gp_path_argmax_kernel<T, 16>; break;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)(bs * a.groups)), dim3(PNT), 0, stream, g);
    const int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(gp_path_argmax_merge_kernel<T>, dim3((unsigned)rows), dim3(PNT), 0, stream, g);
    return launch_status();
}

}  // namespace
}  // namespace pacoh

using namespace pacoh;

extern "C" int pacoh_gp_path_fit(const void* zs, const void* resid, const void* X, const int32_t* info,
                                 const void* outputscale, const void* noise, const void* omega, const void* phase,
                                 const void* w, const void* eps, void* v,
                                 int B, int P, int n, int cap, int S, int D, int f, int dtype, void* stream) {
    if (check_dtype(dtype)) return PACOH_EDTYPE;
    const int rc = path_common(B, P, n, cap, S, D, f, dtype);
    if (rc) return rc;
    if (!zs || !resid || !X || !info || !noise || !omega || !phase || !w || !eps || !v) return PACOH_EINVAL;
    if (dtype == PACOH_F32)
        return path_fit_entry<float>(zs, resid, X, info, outputscale, noise, omega, phase, w, eps, v, B, P, n, cap, S, D, f,
                                     (hipStream_t)stream);
    return path_fit_entry<double>(zs, resid, X, info, outputscale, noise, omega, phase, w, eps, v, B, P, n, cap, S, D, f,
                                  (hipStream_t)stream);
}

extern "C" int pacoh_gp_path_eval(const void* zs, const void* v, const void* w, const int32_t* info,
                                  const void* omega, const void* phase, const void* z_tst, int zt_div,
                                  const void* mean_tst, int mean_mode, const void* lengthscale, const void* outputscale, void* out,
                                  int B, int P, int n, int cap, int S, int D, int m, int f, int dtype, void* stream) {
    if (check_dtype(dtype)) return PACOH_EDTYPE;
    if (zt_div <= 0) return PACOH_EINVAL;
    const int rc = path_common(B, P, n, cap, S, D, f, dtype);
    if (rc) return rc;
    if (m < 1) return PACOH_ELIMIT;
    if (!zs || !v || !w || !info || !omega || !phase || !z_tst || !lengthscale || !out) return PACOH_EINVAL;
    if (mean_mode != PACOH_MEAN_ZERO && !mean_tst) return PACOH_EINVAL;
    if (dtype == PACOH_F32)
        return path_eval_entry<float>(zs, v, w, info, omega, phase, z_tst, zt_div, mean_tst, mean_mode, lengthscale, outputscale, out,
                                      B, P, n, cap, S, D, m, f, (hipStream_t)stream);
    return path_eval_entry<double>(zs, v, w, info, omega, phase, z_tst, zt_div, mean_tst, mean_mode, lengthscale, outputscale, out,
                                   B, P, n, cap, S, D, m, f, (hipStream_t)stream);
}

extern "C" size_t pacoh_gp_path_argmax_workspace_bytes(int B, int S, int m, int strips, int dtype) {
    if (check_dtype(dtype) || B <= 0 || S < 1 || m < 1 || strips < 0) return 0;
    return argmax_pairs(B, S, m, strips) * (sizeof(int64_t) + (dtype == PACOH_F32 ? sizeof(float) : sizeof(double)));
}

extern "C" int pacoh_gp_path_argmax(const void* zs, const void* v, const void* w, const int32_t* info,
                                    const void* omega, const void* phase, const void* z_tst, int zt_div,
                                    const void* mean_tst, int mean_mode, const void* lengthscale, const void* outputscale,
                                    const uint8_t* mask, void* best_val, int64_t* best_idx, void* workspace, size_t workspace_bytes,
                                    int B, int P, int n, int cap, int S, int D, int m, int f, int64_t idx_base, int largest, int first,
                                    int strips, int dtype, void* stream) {
    if (check_dtype(dtype)) return PACOH_EDTYPE;
    if (zt_div <= 0) return PACOH_EINVAL;
    const int rc = path_common(B, P, n, cap, S, D, f, dtype);
    if (rc) return rc;
    if (m < 1) return PACOH_ELIMIT;
    if (strips < 0 || idx_base < 0 || (largest != 0 && largest != 1) || (first != 0 && first != 1)) return PACOH_EINVAL;
    if (!zs || !v || !w || !info || !omega || !phase || !z_tst || !lengthscale || !best_val || !best_idx || !workspace)
        return PACOH_EINVAL;
    if (mean_mode != PACOH_MEAN_ZERO && !mean_tst) return PACOH_EINVAL;
    if (workspace_bytes < pacoh_gp_path_argmax_workspace_bytes(B, S, m, strips, dtype)) return PACOH_EINVAL;
    if (dtype == PACOH_F32)
        return path_argmax_entry<float>(zs, v, w, info, omega, phase, z_tst, zt_div, mean_tst, mean_mode, lengthscale, outputscale, mask,
                                        best_val, best_idx, workspace, B, P, n, cap, S, D, m, f, idx_base, largest, first, strips,
                                        (hipStream_t)stream);
    return path_argmax_entry<double>(zs, v, w, info, omega, phase, z_tst, zt_div, mean_tst, mean_mode, lengthscale, outputscale, mask,
                                     best_val, best_idx, workspace, B, P, n, cap, S, D, m, f, idx_base, largest, first, strips,
                                     (hipStream_t)stream);
}

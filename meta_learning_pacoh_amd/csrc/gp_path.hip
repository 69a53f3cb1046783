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

template <typename T, int FP>
__global__ void __launch_bounds__(PNT) gp_path_eval_kernel(PathEvalArgs<T> a) {
    constexpr int MAXR = CMf<T>::MAXT * 16;
    __shared__ __attribute__((aligned(32))) T Bs[PS][PKP];       // [draw][column of the chunk]; the output tile [draw][test point] at the end
    __shared__ T omL[PK * FP];
    __shared__ T phL[PK];
    __shared__ T zsL[MAXR * FP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4, l15 = lane & 15;
    const int grp = (int)(blockIdx.x % (unsigned)a.groups);
    const unsigned bt = blockIdx.x / (unsigned)a.groups;
    const int tile = (int)(bt % (unsigned)a.tiles);
    const long b = bt / (unsigned)a.tiles;
    const int p = (int)(b % a.P);
    const int n = a.n, cap = a.cap, m = a.m, f = a.f, S = a.S, D = a.D;
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
    const T* zsg = a.zs + b * (long)cap * f;
    for (int e = tid; e < MAXR * FP; e += PNT) {
        const int j = e / FP, c = e - j * FP;
        zsL[e] = (j < n && c < f) ? zsg[(long)j * f + c] : T(0);
    }
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
        __syncthreads();                             // zsL staged (first chunk); the previous chunk has been consumed
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
    // ---- the output tile through LDS: [draw][test point], so that a draw's 64 test points leave as one contiguous row ---------------
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
    for (int e = tid; e < NDT * 16 * PT; e += PNT) {
        const int s = e >> 6, t = e & 63;
        if (s < ns && t0 + t < m) {
            T mt = 0;
            if (a.mean_mode == PACOH_MEAN_VECTOR) mt = a.mean_tst[b * m + t0 + t];
            else if (a.mean_mode == PACOH_MEAN_CONST) mt = a.mean_tst[p];
            og[(long)s * m + t] = mt + Bs[s][t];
        }
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

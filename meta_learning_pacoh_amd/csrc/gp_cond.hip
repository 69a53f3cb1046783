// A conditioned GP posterior kept between calls: condition once, predict many times, append points.
// State of one problem with capacity cap (include/pacoh_gp.h): zs [cap,f] the context features divided by the lengthscales,
// resid [cap] = y - mean, X [cap,cap] row-major with row i < n = row i of L^-1 (K + j I = L L^T, K = os k(Z,Z) + noise I, j the jitter
// of the rung in info), alpha [cap] = (K + j I)^-1 resid, info.  Nothing above the diagonal of X and no row >= n is ever written.
// Upstream counterpart: gpytorch's prediction-strategy caches (mean_cache, covar_cache) and ExactGP.get_fantasy_model.
//
//   pacoh_gp_condition     the pipeline of gp_loo.hip (its phases are DUPLICATED here, not shared: gp_loo.hip stays as it is): Gram in
//                          LDS -> Cholesky with the jitter ladder -> X = L^-1 in place -> u = X r -> alpha = X^T u, then the state is
//                          written.  Same mapping (GS = pow2ceil(n) lanes per problem, lane i owns row i) and the same LDS plan, hence
//                          the same size limit.
//   pacoh_gp_cond_predict  mu = m* + K* alpha, var = os + noise - |X k*|^2.  Grid = problems x tiles of 64 test points; a workgroup of
//                          four waves, 16 test points each.  V = K* X^T on the matrix cores (v_mfma_f32_16x16x4_f32 /
//                          v_mfma_f64_16x16x4_f64): the A operand K*[16, 16-slab] is computed on the fly in registers from the test
//                          features and zs (LDS), the B operand is X staged slab by slab (16 columns, the rows at or below the diagonal
//                          only) in LDS; the column tiles above the diagonal are skipped.  Accumulators: one 16 x 16 tile per 16 context
//                          points (12 tiles fp32, 9 fp64).  Row norms and the alpha dot products are reduced with lane shuffles.
//   pacoh_gp_cond_append   the bordered update, one workgroup per problem, the k points in order; X is read from L2 (a wave per row
//                          for v = X k, a thread per column for v^T X), LDS holds vectors only.  alpha lives in LDS during the launch
//                          and is written back only when every point went in, so a refused problem keeps its rows < n as they were.
#include "common.h"

namespace pacoh {
namespace {

// ================================================================================================================== condition
template <typename T>
struct CondArgs {
    const T* z; int z_div;
    const T* mean; int mean_mode;
    const T* y; int y_div;
    const T* ls; const T* os; const T* noise;
    T* zs; T* resid; T* X; T* alpha; int32_t* info;
    int B, P, n, cap, f, GS, G, LD;
    int kind;
    unsigned per_group;
};

// LDS elements of one group, the plan of gp_loo.hip: L / X [n, LD] | scaled features [n, FP] | residual r | column buffers c0, c1
// (later u) | 1 / L_kk | 16 words of scratch
template <typename T> __host__ __device__ inline unsigned cond_group_elems(int n, int LD, int FP) {
    unsigned e = (unsigned)n * LD + (unsigned)((n * FP + 3) & ~3) + 4u * LD + 16u;
    return (e + 3u) & ~3u;
}

template <typename T> __device__ __forceinline__ void cond_zero_row(T* row, int LD) {
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    V zero;
    if constexpr (W == 4) { zero.x = 0; zero.y = 0; zero.z = 0; zero.w = 0; } else { zero.x = 0; zero.y = 0; }
    V* r = reinterpret_cast<V*>(row);
    for (int v = 0; v < LD / W; ++v) r[v] = zero;
}

// jitter of ladder rung r (0: none), multiplied up in T exactly as the ladder does
template <typename T> __device__ __forceinline__ T rung_jitter(int rung) {
    if (rung <= 0) return T(0);
    T j = sizeof(T) == 4 ? T(1e-6) : T(1e-8);
    for (int q = 1; q < rung; ++q) j *= T(10);
    return j;
}

template <typename T, int FP>
__global__ void __launch_bounds__(256) gp_condition_kernel(CondArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* smem = reinterpret_cast<T*>(smem_raw);

    const int tid = threadIdx.x, GS = a.GS;
    const int g = tid / GS, i = tid - g * GS;
    const int n = a.n, LD = a.LD, f = a.f, cap = a.cap;
    const long b = (long)blockIdx.x * a.G + g;
    const bool live = b < a.B;
    const int p = live ? (int)(b % a.P) : 0;

    T* Lmat = smem + (size_t)g * a.per_group;
    T* zf = Lmat + (size_t)n * LD;
    T* rvec = zf + ((n * FP + 3) & ~3);
    T* c0 = rvec + LD;
    T* c1 = c0 + LD;
    T* invd = c1 + LD;
    T* red = invd + LD;          // [8] failure flag
    T* myrow = Lmat + (size_t)(i < n ? i : 0) * LD;

    T ls[FP];
#pragma unroll
    for (int c = 0; c < FP; ++c) ls[c] = (live && c < f) ? a.ls[(long)p * f + c] : T(1);
    const T os = (live && a.os) ? a.os[p] : T(1);
    const T noise = live ? a.noise[p] : T(1);
    T zs[FP];
#pragma unroll
    for (int c = 0; c < FP; ++c) zs[c] = 0;
    T ri = 0;
    if (live && i < n) {
        const T* zp = a.z + ((b / a.z_div) * n + i) * (long)f;
#pragma unroll
        for (int c = 0; c < FP; ++c) if (c < f) zs[c] = zp[c] / ls[c];
        T mi = 0;
        if (a.mean_mode == PACOH_MEAN_VECTOR) mi = a.mean[b * n + i];
        else if (a.mean_mode == PACOH_MEAN_CONST) mi = a.mean[p];
        ri = a.y[(b / a.y_div) * n + i] - mi;
    }
    if (i < n) {
#pragma unroll
        for (int c = 0; c < FP; ++c) zf[i * FP + c] = zs[c];
    }
    for (int q = i; q < LD; q += GS) { rvec[q] = T(0); c0[q] = T(0); c1[q] = T(0); }

    // ---- Cholesky with the psd_safe_cholesky jitter ladder ------------------------------------------------------------------------
    const T jitter_base = sizeof(T) == 4 ? T(1e-6) : T(1e-8);
    int my_info = -1;
    bool active = true;          // uniform per group
    T jitter = 0;
    for (int attempt = 0; attempt < 4; ++attempt) {
        if (active && i < n) cond_zero_row<T>(myrow, LD);
        if (i == 0) red[8] = 0;
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            T acc = 0;
            if (active && i >= k && i < n) {
                T s = 0;
#pragma unroll
                for (int c = 0; c < FP; ++c) { T d = zs[c] - zf[k * FP + c]; s = fma(d, d, s); }
                T aik = os * kern_val<T>(a.kind, s);
                if (i == k) aik += noise + jitter;
                acc = aik - dot_rows<T>(myrow, Lmat + (size_t)k * LD, 0, k);
                if (i == k) {
                    if (!(acc > T(0))) { red[8] = 1; acc = 1; }
                    T d = t_sqrt<T>(acc);
                    invd[k] = T(1) / d;
                    myrow[k] = d;
                }
            }
            __syncthreads();
            if (active && i > k && i < n) myrow[k] = acc * invd[k];
            __syncthreads();
        }
        bool failed = active && (red[8] != T(0));
        if (active && !failed) { my_info = attempt; active = false; }
        int any = __syncthreads_or(failed ? 1 : 0);
        if (!any) break;
        jitter = jitter_base;
        for (int q = 0; q < attempt; ++q) jitter *= T(10);
    }
    const bool ok = my_info >= 0;
    if (live && i == 0) a.info[b] = my_info;

    // ---- X = L^-1 in place, columns n-1 .. 0 (two alternating column buffers: one barrier per column, see gp_loo.hip) ------------
    if (i < n) rvec[i] = ri;
    for (int j = n - 1; j >= 0; --j) {
        T* cj = (j & 1) ? c1 : c0;
        if (i > j && i < n) cj[i] = myrow[j];
        __syncthreads();
        if (i > j && i < n) myrow[j] = -invd[j] * dot_rows<T>(myrow, cj, j + 1, i + 1);
        else if (i == j) myrow[j] = invd[j];
    }
    // ---- u = X r, alpha = X^T u ---------------------------------------------------------------------------------------------------
    T ui = 0;
    if (i < n) ui = dot_rows<T>(myrow, rvec, 0, i + 1);
    __syncthreads();             // every row of X complete; c0 / c1 no longer read
    if (i < n) c0[i] = ui;
    __syncthreads();
    T ai = 0;
    if (i < n)
        for (int r = i; r < n; ++r) ai = fma(Lmat[(size_t)r * LD + i], c0[r], ai);
    // ---- the state ----------------------------------------------------------------------------------------------------------------
    if (live && i < n) {
        T* zo = a.zs + (b * cap + i) * (long)f;
#pragma unroll
        for (int c = 0; c < FP; ++c) if (c < f) zo[c] = zs[c];
        a.resid[b * cap + i] = ri;
        a.alpha[b * cap + i] = ok ? ai : T(NAN);
    }
    if (live && ok) {            // row r, entries 0 .. r: consecutive lanes, consecutive addresses
        T* Xo = a.X + b * (long)cap * cap;
        for (int r = i; r < n; ++r) Xo[(long)r * cap + i] = Lmat[(size_t)r * LD + i];
    }
}

inline int pow2ceil8(int n) { int g = 8; while (g < n) g <<= 1; return g; }

constexpr size_t COND_LDS_MAX = 160u * 1024u - 256u;

int cond_max_n(int dtype) { return pacoh_gp_loo_max_n(dtype); }      // the same LDS plan as gp_loo.hip: the same limit

template <typename T>
int launch_condition(CondArgs<T> a, hipStream_t stream) {
    const int FP = a.f <= 2 ? 2 : (a.f <= 4 ? 4 : (a.f <= 8 ? 8 : 16));
    a.GS = pow2ceil8(a.n);
    a.G = a.GS >= 64 ? 1 : 64 / a.GS;
    a.LD = lds_ld<T>(a.n);
    a.per_group = cond_group_elems<T>(a.n, a.LD, FP);
    const size_t lds = (size_t)a.per_group * a.G * sizeof(T);
    if (lds > COND_LDS_MAX) return PACOH_ELIMIT;
    const int threads = a.GS >= 64 ? a.GS : 64;
    const long blocks = ((long)a.B + a.G - 1) / a.G;
    if (blocks > 0x7fffffffL) return PACOH_ELIMIT;
    void (*kern)(CondArgs<T>) = nullptr;
    static std::atomic<uint64_t> opted[4];
    int slot;
    switch (FP) {
        case 2: kern = gp_condition_kernel<T, 2>; slot = 0; break;
        case 4: kern = gp_condition_kernel<T, 4>; slot = 1; break;
        case 8: kern = gp_condition_kernel<T, 8>; slot = 2; break;
        default: kern = gp_condition_kernel<T, 16>; slot = 3; break;
    }
    if (lds > 64u * 1024u) {
        const int rc = lds_opt_in(reinterpret_cast<const void*>(kern), (int)COND_LDS_MAX, opted[slot]);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(threads), lds, stream, a);
    return launch_status();
}

// ==================================================================================================================== predict
constexpr int PT = 64;                  // test points per workgroup (4 waves x 16)
constexpr int PK = 16;                  // columns of X per staged slab (4 MFMA k-steps)
constexpr int PNT = 256;

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

template <typename T>
struct CondPredArgs {
    const T* zs; const T* X; const T* alpha; const int32_t* info;
    const T* z_tst; int zt_div; const T* mean_tst; int mean_mode;
    const T* ls; const T* os; const T* noise;
    T* mu; T* var;
    int B, P, n, cap, m, f, kind, tiles;
};

template <typename T, int FP>
__global__ void __launch_bounds__(PNT) gp_cond_predict_kernel(CondPredArgs<T> a) {
    constexpr int MAXT = CMf<T>::MAXT, MAXR = MAXT * 16;
    __shared__ T Xs[MAXR][PK + 1];
    __shared__ T zsL[MAXR * FP];
    __shared__ T alL[MAXR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4, l15 = lane & 15;
    const int tile = (int)(blockIdx.x % (unsigned)a.tiles);
    const long b = blockIdx.x / (unsigned)a.tiles;
    const int p = (int)(b % a.P);
    const int n = a.n, cap = a.cap, m = a.m, f = a.f;
    const int s0 = tile * PT;

    if (a.info[b] < 0) {                             // (uniform per workgroup)
        const int s = s0 + tid;
        if (tid < PT && s < m) {
            a.mu[b * m + s] = T(NAN);
            if (a.var) a.var[b * m + s] = T(NAN);
        }
        return;
    }
    const T* zsg = a.zs + b * (long)cap * f;
    for (int e = tid; e < MAXR * FP; e += PNT) {
        const int j = e / FP, c = e - j * FP;
        zsL[e] = (j < n && c < f) ? zsg[(long)j * f + c] : T(0);
    }
    for (int e = tid; e < MAXR; e += PNT) alL[e] = e < n ? a.alpha[b * cap + e] : T(0);

    // the A operand's row of this lane: test point sa, features divided by the lengthscales as gp_small.hip does
    const int sa = s0 + 16 * wave + l15;
    const T os = a.os ? a.os[p] : T(1);
    T zt[FP];
#pragma unroll
    for (int c = 0; c < FP; ++c) zt[c] = 0;
    if (sa < m) {
        const T* zp = a.z_tst + ((b / a.zt_div) * m + sa) * (long)f;
#pragma unroll
        for (int c = 0; c < FP; ++c) if (c < f) zt[c] = zp[c] / a.ls[(long)p * f + c];
    }
    const bool wave_live = s0 + 16 * wave < m;
    using Acc = typename CMf<T>::acc;
    Acc acc[MAXT];
#pragma unroll
    for (int ct = 0; ct < MAXT; ++ct) acc[ct] = Acc{0, 0, 0, 0};
    T mu_part = 0;
    const int NT = (n + 15) >> 4;
    const T* Xg = a.X + b * (long)cap * cap;
    __syncthreads();                                 // zsL, alL staged
    for (int kt = 0; kt < NT; ++kt) {
        const int k0 = kt * PK;
        // K*[sa, k0 + 4 q + kk], kk = 0..3: MFMA step kk contracts the four context points {k0 + 4 q + kk : q = 0..3} -- the k order
        // inside a slab is permuted alike for A and B
        T av[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int k = k0 + 4 * q + kk;           // < MAXR
            T s2 = 0;
#pragma unroll
            for (int c = 0; c < FP; ++c) { T d = zt[c] - zsL[k * FP + c]; s2 = fma(d, d, s2); }
            av[kk] = k < n ? os * kern_val<T>(a.kind, s2) : T(0);
            mu_part = fma(av[kk], alL[k], mu_part);
        }
        __syncthreads();                             // the previous slab has been consumed
        const int rows = NT * 16 - k0;               // rows k0 .. 16 NT - 1: the tiles above the diagonal are never staged
        for (int e = tid; e < rows * PK; e += PNT) {
            const int i = k0 + (e >> 4), kc = e & 15, k = k0 + kc;
            Xs[i][kc] = (i < n && k <= i) ? Xg[(long)i * cap + k] : T(0);
        }
        __syncthreads();
        if (wave_live) {
#pragma unroll
            for (int ct = 0; ct < MAXT; ++ct) {
                if (ct >= kt && ct < NT) {           // (uniform)
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) acc[ct] = CMf<T>::mma(av[kk], Xs[16 * ct + l15][4 * q + kk], acc[ct]);
                }
            }
        }
    }
    if (!wave_live) return;
    // ---- |V_s|^2 over the context (register r of every tile is one test point; the 16 lanes of a quarter hold 16 columns) ----------
    T ss[4] = {0, 0, 0, 0};
#pragma unroll
    for (int ct = 0; ct < MAXT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) ss[r] = fma(acc[ct][r], acc[ct][r], ss[r]);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        for (int d = 1; d < 16; d <<= 1) ss[r] += shfl_xor_t<T>(ss[r], d);
    mu_part += shfl_xor_t<T>(mu_part, 16);
    mu_part += shfl_xor_t<T>(mu_part, 32);
    if (a.var && l15 == 0) {
        const T noise = a.noise[p];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int s = s0 + 16 * wave + CMf<T>::row(lane, r);
            if (s < m) a.var[b * m + s] = os + noise - ss[r];
        }
    }
    if (q == 0 && sa < m) {
        T mt = 0;
        if (a.mean_mode == PACOH_MEAN_VECTOR) mt = a.mean_tst[b * m + sa];
        else if (a.mean_mode == PACOH_MEAN_CONST) mt = a.mean_tst[p];
        a.mu[b * m + sa] = mt + mu_part;
    }
}

template <typename T>
int launch_cond_predict(CondPredArgs<T> a, hipStream_t stream) {
    if ((a.cap + 15) / 16 > CMf<T>::MAXT) return PACOH_ELIMIT;
    a.tiles = (a.m + PT - 1) / PT;
    const long blocks = (long)a.tiles * a.B;
    if (blocks > 0x7fffffffL) return PACOH_ELIMIT;
    const int FP = a.f <= 2 ? 2 : (a.f <= 4 ? 4 : (a.f <= 8 ? 8 : 16));
    void (*kern)(CondPredArgs<T>) = nullptr;
    switch (FP) {
        case 2: kern = gp_cond_predict_kernel<T, 2>; break;
        case 4: kern = gp_cond_predict_kernel<T, 4>; break;
        case 8: kern = gp_cond_predict_kernel<T, 8>; break;
        default: kern = gp_cond_predict_kernel<T, 16>; break;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(PNT), 0, stream, a);
    return launch_status();
}

// ===================================================================================================================== append
constexpr int AV = 192;                 // >= the largest capacity (checked by the launcher)
constexpr int ANT = 256;

template <typename T>
struct CondAppArgs {
    T* zs; T* resid; T* X; T* alpha; const int32_t* info;
    const T* z_new; int zn_div; const T* mean_new; int mean_mode; const T* y_new; int yn_div;
    const T* ls; const T* os; const T* noise;
    int32_t* fail;
    int B, P, n, cap, k, f, kind;
};

template <typename T> __device__ __forceinline__ T block_sum4(T v, T* red, int tid) {
    v = subwave_sum<T>(v, 64);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

template <typename T>
__global__ void __launch_bounds__(ANT) gp_cond_append_kernel(CondAppArgs<T> a) {
    __shared__ T kL[AV], vL[AV], xr[AV], alL[AV], rsL[AV], zq[PACOH_MAX_FEATURES], red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long b = blockIdx.x;
    const int p = (int)(b % a.P);
    const int n = a.n, cap = a.cap, f = a.f;
    const int rung = a.info[b];
    if (rung < 0) return;                            // never conditioned: skipped
    const T os = a.os ? a.os[p] : T(1);
    const T kappa = os + (a.noise[p] + rung_jitter<T>(rung));
    T* zsb = a.zs + b * (long)cap * f;
    T* Xb = a.X + b * (long)cap * cap;
    for (int i = tid; i < n; i += ANT) { alL[i] = a.alpha[b * cap + i]; rsL[i] = a.resid[b * cap + i]; }

    for (int t = 0; t < a.k; ++t) {
        const int qn = n + t;                        // the index the new point takes
        __syncthreads();                             // the previous point's row of X and of zs is in memory, its vectors are consumed
        if (tid < f) zq[tid] = a.z_new[((b / a.zn_div) * a.k + t) * (long)f + tid] / a.ls[(long)p * f + tid];
        __syncthreads();
        for (int i = tid; i < qn; i += ANT) {
            T s2 = 0;
            for (int c = 0; c < f; ++c) { T d = zq[c] - zsb[(long)i * f + c]; s2 = fma(d, d, s2); }
            kL[i] = os * kern_val<T>(a.kind, s2);
        }
        __syncthreads();
        for (int i = wave; i < qn; i += ANT / 64) {  // v = X k: a wave per row
            T s = 0;
            for (int j = lane; j <= i; j += 64) s = fma(Xb[(long)i * cap + j], kL[j], s);
            s = subwave_sum<T>(s, 64);
            if (lane == 0) vL[i] = s;
        }
        __syncthreads();
        T part = 0;
        for (int i = tid; i < qn; i += ANT) part = fma(vL[i], vL[i], part);
        const T s2 = kappa - block_sum4<T>(part, red, tid);
        if (!(s2 > T(0))) {                          // (uniform) refused: alpha is not written back, rows < n stay as they were
            if (tid == 0) a.fail[b] = 1;
            return;
        }
        const T inv = T(1) / t_sqrt<T>(s2);
        for (int j = tid; j < qn; j += ANT) {        // v^T X: a thread per column
            T w = 0;
            for (int i = j; i < qn; ++i) w = fma(vL[i], Xb[(long)i * cap + j], w);
            xr[j] = -w * inv;
        }
        if (tid == 0) {
            xr[qn] = inv;
            T mq = 0;
            if (a.mean_mode == PACOH_MEAN_VECTOR) mq = a.mean_new[b * a.k + t];
            else if (a.mean_mode == PACOH_MEAN_CONST) mq = a.mean_new[p];
            rsL[qn] = a.y_new[(b / a.yn_div) * a.k + t] - mq;
            alL[qn] = T(0);
        }
        __syncthreads();
        part = 0;
        for (int j = tid; j <= qn; j += ANT) part = fma(xr[j], rsL[j], part);
        const T u = block_sum4<T>(part, red, tid);
        for (int j = tid; j <= qn; j += ANT) {
            alL[j] = fma(xr[j], u, alL[j]);
            Xb[(long)qn * cap + j] = xr[j];
        }
        if (tid < f) zsb[(long)qn * f + tid] = zq[tid];
        if (tid == 0) a.resid[b * cap + qn] = rsL[qn];
    }
    __syncthreads();
    for (int i = tid; i < n + a.k; i += ANT) a.alpha[b * cap + i] = alL[i];
}

// the checks the three entry points share: 0, or the error code
int cond_common(int B, int P, int n, int cap, int f_arg, int dtype) {
    if (B <= 0 || P <= 0 || n <= 0 || cap <= 0 || features_of(f_arg) <= 0) return PACOH_EINVAL;
    if (features_of(f_arg) > PACOH_MAX_FEATURES || !family_known(kernel_of(f_arg))) return PACOH_ELIMIT;
    if (n > cap || cap > cond_max_n(dtype) || cap > AV) return PACOH_ELIMIT;
    return PACOH_OK;
}

template <typename T>
int condition_entry(const void* z, int z_div, const void* mean, int mean_mode, const void* y, int y_div, const void* ls, const void* os,
                    const void* noise, void* zs, void* resid, void* X, void* alpha, int32_t* info, int B, int P, int n, int cap, int f,
                    hipStream_t stream) {
    CondArgs<T> a = {};
    a.z = (const T*)z; a.z_div = z_div; a.mean = (const T*)mean; a.mean_mode = mean_mode; a.y = (const T*)y; a.y_div = y_div;
    a.ls = (const T*)ls; a.os = (const T*)os; a.noise = (const T*)noise;
    a.zs = (T*)zs; a.resid = (T*)resid; a.X = (T*)X; a.alpha = (T*)alpha; a.info = info;
    a.B = B; a.P = P; a.n = n; a.cap = cap; a.f = features_of(f); a.kind = kernel_of(f);
    return launch_condition<T>(a, stream);
}

template <typename T>
int cond_predict_entry(const void* zs, const void* X, const void* alpha, const int32_t* info, const void* z_tst, int zt_div,
                       const void* mean_tst, int mean_mode, const void* ls, const void* os, const void* noise, void* mu, void* var,
                       int B, int P, int n, int cap, int m, int f, hipStream_t stream) {
    CondPredArgs<T> a = {};
    a.zs = (const T*)zs; a.X = (const T*)X; a.alpha = (const T*)alpha; a.info = info;
    a.z_tst = (const T*)z_tst; a.zt_div = zt_div; a.mean_tst = (const T*)mean_tst; a.mean_mode = mean_mode;
    a.ls = (const T*)ls; a.os = (const T*)os; a.noise = (const T*)noise; a.mu = (T*)mu; a.var = (T*)var;
    a.B = B; a.P = P; a.n = n; a.cap = cap; a.m = m; a.f = features_of(f); a.kind = kernel_of(f);
    return launch_cond_predict<T>(a, stream);
}

template <typename T>
int cond_append_entry(void* zs, void* resid, void* X, void* alpha, const int32_t* info, const void* z_new, int zn_div,
                      const void* mean_new, int mean_mode, const void* y_new, int yn_div, const void* ls, const void* os,
                      const void* noise, int32_t* fail, int B, int P, int n, int cap, int k, int f, hipStream_t stream) {
    CondAppArgs<T> a = {};
    a.zs = (T*)zs; a.resid = (T*)resid; a.X = (T*)X; a.alpha = (T*)alpha; a.info = info;
    a.z_new = (const T*)z_new; a.zn_div = zn_div; a.mean_new = (const T*)mean_new; a.mean_mode = mean_mode;
    a.y_new = (const T*)y_new; a.yn_div = yn_div; a.ls = (const T*)ls; a.os = (const T*)os; a.noise = (const T*)noise; a.fail = fail;
    a.B = B; a.P = P; a.n = n; a.cap = cap; a.k = k; a.f = features_of(f); a.kind = kernel_of(f);
    if (B > 0x7fffffffL) return PACOH_ELIMIT;
    hipLaunchKernelGGL(gp_cond_append_kernel<T>, dim3((unsigned)B), dim3(ANT), 0, stream, a);
    return launch_status();
}

}  // namespace
}  // namespace pacoh

using namespace pacoh;

extern "C" int pacoh_gp_cond_max_n(int dtype) {
    if (check_dtype(dtype)) return PACOH_EDTYPE;
    return cond_max_n(dtype);
}

extern "C" int pacoh_gp_condition(const void* z, int z_div, const void* mean, int mean_mode, const void* y, int y_div,
                                  const void* lengthscale, const void* outputscale, const void* noise,
                                  void* zs, void* resid, void* X, void* alpha, int32_t* info,
                                  int B, int P, int n, int cap, int f, int dtype, void* stream) {
    if (check_dtype(dtype)) return PACOH_EDTYPE;
    if (z_div <= 0 || y_div <= 0) return PACOH_EINVAL;
    const int rc = cond_common(B, P, n, cap, f, dtype);
    if (rc) return rc;
    if (!z || !y || !lengthscale || !noise || !zs || !resid || !X || !alpha || !info) return PACOH_EINVAL;
    if (mean_mode != PACOH_MEAN_ZERO && !mean) return PACOH_EINVAL;
    if (dtype == PACOH_F32)
        return condition_entry<float>(z, z_div, mean, mean_mode, y, y_div, lengthscale, outputscale, noise, zs, resid, X, alpha, info,
                                      B, P, n, cap, f, (hipStream_t)stream);
    return condition_entry<double>(z, z_div, mean, mean_mode, y, y_div, lengthscale, outputscale, noise, zs, resid, X, alpha, info,
                                   B, P, n, cap, f, (hipStream_t)stream);
}

extern "C" int pacoh_gp_cond_predict(const void* zs, const void* X, const void* alpha, const int32_t* info,
                                     const void* z_tst, int zt_div, const void* mean_tst, int mean_mode,
                                     const void* lengthscale, const void* outputscale, const void* noise, void* mu, void* var,
                                     int B, int P, int n, int cap, int m, int f, int dtype, void* stream) {
    if (check_dtype(dtype)) return PACOH_EDTYPE;
    if (zt_div <= 0 || m <= 0) return PACOH_EINVAL;
    const int rc = cond_common(B, P, n, cap, f, dtype);
    if (rc) return rc;
    if (!zs || !X || !alpha || !info || !z_tst || !lengthscale || !noise || !mu) return PACOH_EINVAL;
    if (mean_mode != PACOH_MEAN_ZERO && !mean_tst) return PACOH_EINVAL;
    if (dtype == PACOH_F32)
        return cond_predict_entry<float>(zs, X, alpha, info, z_tst, zt_div, mean_tst, mean_mode, lengthscale, outputscale, noise, mu, var,
                                         B, P, n, cap, m, f, (hipStream_t)stream);
    return cond_predict_entry<double>(zs, X, alpha, info, z_tst, zt_div, mean_tst, mean_mode, lengthscale, outputscale, noise, mu, var,
                                      B, P, n, cap, m, f, (hipStream_t)stream);
}

extern "C" int pacoh_gp_cond_append(void* zs, void* resid, void* X, void* alpha, const int32_t* info,
                                    const void* z_new, int zn_div, const void* mean_new, int mean_mode, const void* y_new, int yn_div,
                                    const void* lengthscale, const void* outputscale, const void* noise, int32_t* fail,
                                    int B, int P, int n, int cap, int k, int f, int dtype, void* stream) {
    if (check_dtype(dtype)) return PACOH_EDTYPE;
    if (zn_div <= 0 || yn_div <= 0 || k <= 0) return PACOH_EINVAL;
    const int rc = cond_common(B, P, n, cap, f, dtype);
    if (rc) return rc;
    if ((long)n + k > cap) return PACOH_ELIMIT;
    if (!zs || !resid || !X || !alpha || !info || !z_new || !y_new || !lengthscale || !noise || !fail) return PACOH_EINVAL;
    if (mean_mode != PACOH_MEAN_ZERO && !mean_new) return PACOH_EINVAL;
    if (dtype == PACOH_F32)
        return cond_append_entry<float>(zs, resid, X, alpha, info, z_new, zn_div, mean_new, mean_mode, y_new, yn_div, lengthscale,
                                        outputscale, noise, fail, B, P, n, cap, k, f, (hipStream_t)stream);
    return cond_append_entry<double>(zs, resid, X, alpha, info, z_new, zn_div, mean_new, mean_mode, y_new, yn_div, lengthscale,
                                     outputscale, noise, fail, B, P, n, cap, k, f, (hipStream_t)stream);
}

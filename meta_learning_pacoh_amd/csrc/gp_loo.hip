// Leave-one-out predictive of the task GPs and its log pseudo-likelihood in ONE launch per batch:
//   features -> Gram (never written to HBM) -> Cholesky with the jitter ladder -> X = L^-1 IN PLACE -> d = diag(K^-1), alpha -> outputs.
// With K = os k(Z,Z) + noise I = L L^T, alpha = K^-1 (y - m), d_i = [K^-1]_ii (Rasmussen & Williams 5.4.2, eqs. 5.10-5.12):
//   mu_loo[i] = y_i - alpha_i / d_i      var_loo[i] = 1 / d_i      lpd = (1/n) sum_i log N(y_i; mu_loo[i], var_loo[i])
// Upstream counterpart: gpytorch.mlls.LeaveOneOutPseudoLikelihood (which forms K^-1 by a dense solve against the identity).
//
// Mapping (that of gp_small.hip): one group of GS = pow2ceil(n) lanes per GP problem, lane i owns row i; n <= 32 packs 64/GS problems
// into one wave, larger n is one problem per workgroup of GS threads.  Every O(n^3) phase is a dot product of the lane's own LDS row
// (ds_read_b128, conflict-free by the leading dimension of lds_ld()) with one vector broadcast to all lanes:
//   Cholesky (left-looking)     acc_i = A_ik - <L_i, L_k>                      A_ik computed on the fly from z
//   X = L^-1 in place           X_ij  = -<X_i[j+1..i], L_[j+1..i],j> / L_jj     columns j = n-1 .. 0 (the unblocked trti2 order): column j
//                               of L, still untouched, is first copied into a vector, then overwritten row by row with column j of X
//   u = X r                     u_i   = <X_i, r>
//   d_i = sum_r X_ri^2, alpha_i = sum_r X_ri u_r      column reads: consecutive lanes, consecutive addresses
// A second n x n matrix does not exist: at n = 128 in fp64 L alone is 128 x 130 x 8 B = 133 KB of the 160 KB LDS.
// If the Cholesky needed jitter (info = 1..3) all quantities are those of the JITTERED matrix K + j I.
#include "common.h"

namespace pacoh {
namespace {

template <typename T>
struct LooArgs {
    const T* z; int z_div;
    const T* mean; int mean_mode;
    const T* y; int y_div;
    const T* ls; const T* os; const T* noise;
    const int32_t* n_valid;
    T* mu; T* var; T* lpd; int32_t* info;
    int B, P, n, f, GS, G, LD;
    int kind;             // kernel family (PACOH_KERNEL_*), decoded from the f argument of the entry point
    unsigned per_group;   // LDS elements per group
};

// LDS elements of one group: L / X [n, LD] | scaled features [n, FP] | residual r | column buffers c0, c1 (later u) | 1 / L_kk | 16 words
// of reduction scratch.  Host plan and kernel carve from this one formula; every offset is a multiple of 16 bytes.
template <typename T> __host__ __device__ inline unsigned loo_group_elems(int n, int LD, int FP) {
    unsigned e = (unsigned)n * LD + (unsigned)((n * FP + 3) & ~3) + 4u * LD + 16u;
    return (e + 3u) & ~3u;
}

// sum over the group's lanes; GS > 64 is one group per workgroup, so the barriers are uniform
template <typename T>
__device__ __forceinline__ T group_sum(T v, int GS, int i, T* red) {
    v = subwave_sum<T>(v, GS < 64 ? GS : 64);
    if (GS > 64) {
        __syncthreads();
        if ((i & 63) == 0) red[i >> 6] = v;
        __syncthreads();
        T s = 0;
        for (int q = 0; q < GS / 64; ++q) s += red[q];
        v = s;
    }
    return v;
}

template <typename T> __device__ __forceinline__ void zero_row(T* row, int LD) {
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    V zero;
    if constexpr (W == 4) { zero.x = 0; zero.y = 0; zero.z = 0; zero.w = 0; } else { zero.x = 0; zero.y = 0; }
    V* r = reinterpret_cast<V*>(row);
    for (int v = 0; v < LD / W; ++v) r[v] = zero;
}

template <typename T, int FP>
__global__ void __launch_bounds__(256) gp_loo_kernel(LooArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* smem = reinterpret_cast<T*>(smem_raw);

    const int tid = threadIdx.x, GS = a.GS;
    const int g = tid / GS, i = tid - g * GS;
    const int n = a.n, LD = a.LD, f = a.f;
    const long b = (long)blockIdx.x * a.G + g;
    const bool live = b < a.B;
    const int p = live ? (int)(b % a.P) : 0;
    const long ty = live ? b / a.y_div : 0;
    int nv = 0;
    if (live) { nv = a.n_valid ? a.n_valid[ty] : n; nv = nv < n ? nv : n; nv = nv < 0 ? 0 : nv; }

    T* Lmat = smem + (size_t)g * a.per_group;
    T* zf = Lmat + (size_t)n * LD;
    T* rvec = zf + ((n * FP + 3) & ~3);
    T* c0 = rvec + LD;
    T* c1 = c0 + LD;
    T* invd = c1 + LD;
    T* red = invd + LD;          // [0..3] cross-wave sums, [8] failure flag
    T* myrow = Lmat + (size_t)(i < n ? i : 0) * LD;

    // ---- hyper-parameters of this problem's set p, features pre-divided by the lengthscale, residual ----------------------------
    T ls[FP];
#pragma unroll
    for (int c = 0; c < FP; ++c) ls[c] = (live && c < f) ? a.ls[(long)p * f + c] : T(1);
    const T os = (live && a.os) ? a.os[p] : T(1);
    const T noise = live ? a.noise[p] : T(1);
    T zs[FP];
#pragma unroll
    for (int c = 0; c < FP; ++c) zs[c] = 0;
    T yi = 0, ri = 0;
    if (i < nv) {
        const T* zp = a.z + ((b / a.z_div) * n + i) * (long)f;
#pragma unroll
        for (int c = 0; c < FP; ++c) if (c < f) zs[c] = zp[c] / ls[c];
        T mi = 0;
        if (a.mean_mode == PACOH_MEAN_VECTOR) mi = a.mean[b * n + i];
        else if (a.mean_mode == PACOH_MEAN_CONST) mi = a.mean[p];
        yi = a.y[ty * n + i];
        ri = yi - mi;
    }
    if (i < n) {
#pragma unroll
        for (int c = 0; c < FP; ++c) zf[i * FP + c] = zs[c];
    }
    // r, c0, c1 zero-filled to LD (the dot products run to vector boundaries); lane i of the group fills its share
    for (int q = i; q < LD; q += GS) { rvec[q] = T(0); c0[q] = T(0); c1[q] = T(0); }

    // ---- Cholesky with the psd_safe_cholesky jitter ladder (rows beyond n_valid: identity block) ---------------------------------
    const T jitter_base = sizeof(T) == 4 ? T(1e-6) : T(1e-8);
    int my_info = -1;
    bool active = true;          // uniform per group
    T jitter = 0;
    for (int attempt = 0; attempt < 4; ++attempt) {
        if (active && i < n) zero_row<T>(myrow, LD);
        if (i == 0) red[8] = 0;
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            T acc = 0;
            if (active && i >= k && i < n) {
                T aik;
                if (i < nv && k < nv) {
                    T s = 0;
#pragma unroll
                    for (int c = 0; c < FP; ++c) { T d = zs[c] - zf[k * FP + c]; s = fma(d, d, s); }
                    aik = os * kern_val<T>(a.kind, s);
                    if (i == k) aik += noise + jitter;
                } else {
                    aik = (i == k) ? T(1) : T(0);
                }
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
    if (live && i == 0 && a.info) a.info[b] = my_info;

    // ---- X = L^-1 in place, columns n-1 .. 0.  Step j: every lane i > j publishes L_ij (its own row, column j) in the column buffer,
    // then X_ij = -<X_i[j+1..i], buffer[j+1..i]> / L_jj overwrites it.  Two buffers alternate, so one barrier per column is enough: the
    // buffer written at step j was last read at step j + 2, before the barrier of step j + 1.  Entries <= j of a buffer are never
    // written before step j (they are still zero) and X_i is zero beyond i, which is what widening the dot to vector boundaries needs.
    if (i < n) rvec[i] = ri;
    for (int j = n - 1; j >= 0; --j) {
        T* cj = (j & 1) ? c1 : c0;
        if (i > j && i < n) cj[i] = myrow[j];
        __syncthreads();
        if (i > j && i < n) myrow[j] = -invd[j] * dot_rows<T>(myrow, cj, j + 1, i + 1);
        else if (i == j) myrow[j] = invd[j];
    }
    // ---- u = X r ------------------------------------------------------------------------------------------------------------------
    T ui = 0;
    if (i < n) ui = dot_rows<T>(myrow, rvec, 0, i + 1);
    __syncthreads();             // every row of X complete; c0 / c1 no longer read
    if (i < n) c0[i] = ui;
    __syncthreads();
    // ---- d_i = sum_{r >= i} X_ri^2, alpha_i = sum_{r >= i} X_ri u_r (rows >= n_valid are unit rows: they add nothing to i < n_valid) --
    T di = 0, ai = 0;
    if (i < nv) {
        for (int r = i; r < nv; ++r) {
            const T x = Lmat[(size_t)r * LD + i];
            di = fma(x, x, di);
            ai = fma(x, c0[r], ai);
        }
    }
    const T bad = ok ? T(0) : T(NAN);
    const T vi = i < nv ? T(1) / di : T(0);
    const T ei = ai * vi;                                  // y_i - mu_loo[i]
    if (live && i < n) {
        if (a.mu) a.mu[b * n + i] = (i < nv ? yi - ei : T(0)) + bad;
        if (a.var) a.var[b * n + i] = vi + bad;
    }
    if (a.lpd) {                                           // (uniform: no divergent barrier inside group_sum)
        const T LOG2PI = T(1.8378770664093453);
        const T term = i < nv ? T(-0.5) * (LOG2PI - t_log<T>(di) + ai * ei) : T(0);
        const T s = group_sum<T>(term, GS, i, red);
        if (live && i == 0) a.lpd[b] = (nv > 0 ? s / T(nv) : T(0)) + bad;
    }
}

inline int pow2ceil8(int n) { int g = 8; while (g < n) g <<= 1; return g; }

constexpr size_t LOO_LDS_MAX = 160u * 1024u - 256u;      // dynamic LDS: the kernel's 256 bytes of static LDS come on top

template <typename T>
size_t loo_lds_bytes(int n, int FP) {
    const int GS = pow2ceil8(n);
    const int G = GS >= 64 ? 1 : 64 / GS;
    return (size_t)loo_group_elems<T>(n, lds_ld<T>(n), FP) * G * sizeof(T);
}

template <typename T>
int loo_max_n() {
    int best = 0;
    for (int n = 1; n <= 256; ++n)
        if (loo_lds_bytes<T>(n, 16) <= LOO_LDS_MAX) best = n;
    return best;
}

template <typename T>
int launch_gp_loo(LooArgs<T> a, hipStream_t stream) {
    if (a.B <= 0 || a.P <= 0 || a.n <= 0 || a.f <= 0 || a.z_div <= 0 || a.y_div <= 0) return PACOH_EINVAL;
    if (a.f > PACOH_MAX_FEATURES || !family_known(a.kind)) return PACOH_ELIMIT;
    if (!a.z || !a.y || !a.ls || !a.noise) return PACOH_EINVAL;
    if (a.mean_mode != PACOH_MEAN_ZERO && !a.mean) return PACOH_EINVAL;
    if (a.n > loo_max_n<T>()) return PACOH_ELIMIT;
    const int FP = a.f <= 2 ? 2 : (a.f <= 4 ? 4 : (a.f <= 8 ? 8 : 16));
    a.GS = pow2ceil8(a.n);
    a.G = a.GS >= 64 ? 1 : 64 / a.GS;
    a.LD = lds_ld<T>(a.n);
    a.per_group = loo_group_elems<T>(a.n, a.LD, FP);
    const size_t lds = (size_t)a.per_group * a.G * sizeof(T);
    if (lds > LOO_LDS_MAX) return PACOH_ELIMIT;
    const int threads = a.GS >= 64 ? a.GS : 64;
    const long blocks = ((long)a.B + a.G - 1) / a.G;
    if (blocks > 0x7fffffffL) return PACOH_ELIMIT;
    void (*kern)(LooArgs<T>) = nullptr;
    static std::atomic<uint64_t> opted[4];
    int slot;
    switch (FP) {
        case 2: kern = gp_loo_kernel<T, 2>; slot = 0; break;
        case 4: kern = gp_loo_kernel<T, 4>; slot = 1; break;
        case 8: kern = gp_loo_kernel<T, 8>; slot = 2; break;
        default: kern = gp_loo_kernel<T, 16>; slot = 3; break;
    }
    if (lds > 64u * 1024u) {
        const int rc = lds_opt_in(reinterpret_cast<const void*>(kern), (int)LOO_LDS_MAX, opted[slot]);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(threads), lds, stream, a);
    return launch_status();
}

template <typename T>
int gp_loo_entry(const void* z, int z_div, const void* mean, int mean_mode, const void* y, int y_div, const void* ls, const void* os,
                 const void* noise, const int32_t* n_valid, void* mu, void* var, void* lpd, int32_t* info, int B, int P, int n, int f,
                 hipStream_t stream) {
    LooArgs<T> a = {};
    a.z = (const T*)z; a.z_div = z_div; a.mean = (const T*)mean; a.mean_mode = mean_mode;
    a.y = (const T*)y; a.y_div = y_div; a.ls = (const T*)ls; a.os = (const T*)os; a.noise = (const T*)noise;
    a.n_valid = n_valid; a.mu = (T*)mu; a.var = (T*)var; a.lpd = (T*)lpd; a.info = info;
    a.B = B; a.P = P; a.n = n; a.f = features_of(f); a.kind = kernel_of(f);
    return launch_gp_loo<T>(a, stream);
}

}  // namespace
}  // namespace pacoh

using namespace pacoh;

extern "C" int pacoh_gp_loo_max_n(int dtype) {
    if (check_dtype(dtype)) return PACOH_EDTYPE;
    return dtype == PACOH_F32 ? loo_max_n<float>() : loo_max_n<double>();
}

extern "C" int pacoh_gp_loo(const void* z, int z_div, const void* mean, int mean_mode, const void* y, int y_div,
                            const void* lengthscale, const void* outputscale, const void* noise, const int32_t* n_valid,
                            void* mu_loo, void* var_loo, void* lpd, int32_t* info,
                            int B, int P, int n, int f, int dtype, void* stream) {
    if (check_dtype(dtype)) return PACOH_EDTYPE;
    if (!mu_loo && !var_loo && !lpd) return PACOH_EINVAL;
    if (dtype == PACOH_F32)
        return gp_loo_entry<float>(z, z_div, mean, mean_mode, y, y_div, lengthscale, outputscale, noise, n_valid, mu_loo, var_loo, lpd,
                                   info, B, P, n, f, (hipStream_t)stream);
    return gp_loo_entry<double>(z, z_div, mean, mean_mode, y, y_div, lengthscale, outputscale, noise, n_valid, mu_loo, var_loo, lpd,
                                info, B, P, n, f, (hipStream_t)stream);
}

// gp_fwd_reg_kernel: gp_reg_kernel<4, 2, true, false> (gp_reg.hip) with the forward of the step's two per-particle networks as its
// prologue -- one 64-lane wavefront (= one workgroup) per (task, particle) problem of n = 64 points computes the mean and the
// kernel-feature network of ITS 64 rows (one 64-point tile of mlp_fused_fwd_kernel), leaves their outputs in the GP body's LDS
// vectors and runs gp_reg_body on them.  What that removes from an SVGD step: the forward launch with its nearly empty last round of
// workgroups, the launch boundary (a problem no longer waits for the forward of every other problem), and the round trip of
// z [B, 64, f] and the mean [B, 64] through memory.
//
// The arithmetic is that of mlp_fused.hip's forward, operation by operation (f_layer1, f_hidden, tanh_pre, the output layer on the
// vector units and the weights pre-multiplied by TSC), so the stash the unchanged backward reads, z and the mean are the same bits:
//   * the inputs of a 16-point block are the B operand of the first layer's MFMA, lane (r, g) <- x[point r][k = g]: four coalesced
//     256-byte loads per problem, straight into registers (no staging);
//   * the weights are the A operands, lane (r, g) <- W[row 16 ob + r][16 kb + 4 g ..+3], read from the particle's theta row (L2) with
//     TSC applied on load and held in registers for the network's four point blocks: about 50 registers per network.  Rows
//     and columns past a narrower layer, and inputs past d_in, are zero as fused_load_weights pads them (W32 = false; widths of 32 skip
//     the masks);
//   * the point blocks run one after the other, fenced, so that only one block's activations (16 registers) are live;
//   * the top hidden layer goes to the activation stash in mlp_fused.hip's layout (block 4 t + pb of particle p) with the same
//     non-temporal stores; they drain under the GP phase.
// The particle-distance block of the pipelined SVGD step (step_tail.h, svgd_dist_tail), which rides in the forward launch, rides
// here instead, in workgroups behind the problems -- as one wavefront that keeps the partial sums of svgd_dist_block's 256 threads
// apart, so that the distances (and the median bandwidth) stay the same bits.
// Replaces NeuralNetworkVectorized.forward (meta_learn/models.py:295-317, 343-349) + random_gp.py:54-89 as one launch.
#include "gp_reg_body.h"
#include "mlp_act.h"
#include "step_tail.h"
#include "switches.h"

namespace pacoh {

struct FwdGpArgs {
    const float* x;                 // [T, 64, d_in]
    const float* theta; long theta_stride;
    long off_mean, off_kern;        // element offsets of the two networks' blocks in a theta row
    float* stash_mean; float* stash_kern;   // activation stash of either network (mlp_fused.hip: stash_off), nullptr = none
    int d_in, h0, h1;               // (h1: NH == 2 only)
    int nblk;                       // 16-point blocks per particle in the stash
    unsigned n_prob;                // B: workgroups from here on run the distance tail
    SvgdDistTail<float> sv;
};

namespace gpreg {

// the body reads row i's features and prior mean from zf / rv, where the prologue below has left them
struct FwdCtx : KernelCtx {
    static constexpr bool LDS_INPUTS = true;
    // (the body derives its lane indices afresh: shared with the prologue's they stay live across it and spill)
    __device__ __forceinline__ int lane() const { int l = threadIdx.x; asm volatile("" : "+v"(l)); return l; }
};

// svgd_dist_tail (step_tail.h) by ONE wavefront: lane l keeps the running sums of threads l, l + 64, l + 128, l + 192 of
// svgd_dist_block's 256-thread workgroup apart (thread t sums the entries t, t + 256, ... in that order), reduces each over the
// lanes as subwave_sum does and adds the four as the workgroup does: the same bits
__device__ __forceinline__ void dist_tail_wave(const SvgdDistTail<float>& t, int lin, int nlin) {
    const int lane = threadIdx.x;
    if (lin == 0 && lane == 0 && t.counter) *t.counter += 1;
    for (int pair = lin; pair < t.P * t.P; pair += nlin) {
        const int i = pair / t.P, j = pair - i * t.P;
        if (j > i) continue;
        const float* xi = t.X + (long)i * t.D;
        if (t.snap && i == j) {
            for (int d = lane; d < t.D; d += 64) t.snap[(long)i * t.D + d] = xi[d];
            if (lane == 0) t.d2[i * t.P + i] = 0.0f;
            continue;
        }
        const float* xj = t.X + (long)j * t.D;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int d0 = lane; d0 < t.D; d0 += 256) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int d = d0 + 64 * w;
                if (d < t.D) { const float df = xi[d] - xj[d]; acc[w] = fmaf(df, df, acc[w]); }
            }
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) acc[w] = subwave_sum<float>(acc[w], 64);
        if (lane == 0) { const float tot = (acc[0] + acc[1]) + (acc[2] + acc[3]); t.d2[i * t.P + j] = tot; t.d2[j * t.P + i] = tot; }
    }
}

// One network of this problem: theta block `th`, d_out outputs (1: the mean -> rv[point]; else the features -> zf[point * 2 + o]),
// for the four 16-point blocks whose first-layer operands are bx[pb]; top hidden layer -> stash block blk0 + pb (stash != nullptr).
template <int NH, bool W32, bool MEAN>
__device__ __forceinline__ void fwd_net(const float* __restrict__ th, const FwdGpArgs& fa, int d_out, const float (&bx)[4], float* stash,
                                        long blk0, int lane, float* zf, float* rv) {
    const int r = lane & 15, g = lane >> 4;
    const int h0 = W32 ? 32 : fa.h0, d_in = fa.d_in;
    // first layer: H1^T = tanh(W1 x + b1), one MFMA per feature block (k = g covers d_in <= 4)
    float aw1[2];
    f32x4 b1[2];
#pragma unroll
    for (int fb = 0; fb < 2; ++fb) {
        const int o = fb * 16 + r;
        aw1[fb] = ((W32 || o < h0) && g < d_in) ? TSC * th[h0 + o * d_in + g] : 0.0f;
#pragma unroll
        for (int s = 0; s < 4; ++s) { const int q = fb * 16 + 4 * g + s; b1[fb][s] = (W32 || q < h0) ? TSC * th[q] : 0.0f; }
    }
    int src = h0 * (d_in + 1), prev = h0;
    // hidden layer: OUT^T = tanh(W IN^T + b)
    f32x4 aw2[2][2], b2[2];
    if constexpr (NH == 2) {
        const int hl = W32 ? 32 : fa.h1;
#pragma unroll
        for (int ob = 0; ob < 2; ++ob) {
            const int o = ob * 16 + r;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = kb * 16 + 4 * g + j;
                    aw2[ob][kb][j] = (W32 || (o < hl && k < prev)) ? TSC * th[src + hl + o * prev + k] : 0.0f;
                }
#pragma unroll
            for (int s = 0; s < 4; ++s) { const int q = ob * 16 + 4 * g + s; b2[ob][s] = (W32 || q < hl) ? TSC * th[src + q] : 0.0f; }
        }
        src += hl * (prev + 1);
        prev = hl;
    }
    // output layer (vector units): W_out[o][feature fb*16+4g+s], rows >= d_out zero
    constexpr int NO = MEAN ? 1 : 2;
    float w3[NO][2][4], b3[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        b3[o] = o < d_out ? th[src + o] : 0.0f;
#pragma unroll
        for (int fb = 0; fb < 2; ++fb)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = fb * 16 + 4 * g + s;
                w3[o][fb][s] = (o < d_out && (W32 || k < prev)) ? th[src + d_out + o * prev + k] : 0.0f;
            }
    }
#pragma unroll
    for (int pb = 0; pb < 4; ++pb) {
        asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0);      // (one point block's activations live at a time)
        f32x4 HA[2], HB[2];
#pragma unroll
        for (int fb = 0; fb < 2; ++fb) {
            f32x4 acc = mfma_(aw1[fb], bx[pb], b1[fb]);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[s] = tanh_pre(acc[s]);
            HA[fb] = acc;
        }
        if constexpr (NH == 2) {
#pragma unroll
            for (int ob = 0; ob < 2; ++ob) {
                f32x4 acc = b2[ob];
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    acc = mfma_(aw2[ob][kb][0], HA[kb][0], acc); acc = mfma_(aw2[ob][kb][1], HA[kb][1], acc);
                    acc = mfma_(aw2[ob][kb][2], HA[kb][2], acc); acc = mfma_(aw2[ob][kb][3], HA[kb][3], acc);
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[s] = tanh_pre(acc[s]);
                HB[ob] = acc;
            }
            if (stash) {        // mlp_fused.hip, stash_off: particle-major [16-point block][slot = 0 of 1][feature block][lane] f32x4
#pragma unroll
                for (int fb = 0; fb < 2; ++fb)
                    __builtin_nontemporal_store(HB[fb], reinterpret_cast<f32x4*>(stash + ((((blk0 + pb) * 2 + fb) << 8) + (lane << 2))));
            }
        }
        const f32x4 (&HL)[2] = NH == 2 ? HB : HA;
        float v[NO];
#pragma unroll
        for (int o = 0; o < NO; ++o) v[o] = 0.0f;
#pragma unroll
        for (int fb = 0; fb < 2; ++fb)
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int o = 0; o < NO; ++o) v[o] = fmaf(w3[o][fb][s], HL[fb][s], v[o]);
#pragma unroll
        for (int o = 0; o < NO; ++o) { v[o] += __shfl_xor(v[o], 16, 64); v[o] += __shfl_xor(v[o], 32, 64); }      // sum over the four feature groups g
        if (g == 0) {
            if constexpr (MEAN) rv[pb * 16 + r] = v[0] + b3[0];
            else {
                zf[(pb * 16 + r) * 2] = v[0] + b3[0];
                if (d_out > 1) zf[(pb * 16 + r) * 2 + 1] = v[1] + b3[1];
            }
        }
    }
}

}  // namespace gpreg

template <int NH, bool W32>
__global__ void __launch_bounds__(64, 4) gp_fwd_reg_kernel(GpMfmaArgs a, FwdGpArgs fa) {
    if (blockIdx.x >= fa.n_prob) {                        // the SVGD step's distance matrix rides in this launch
        gpreg::dist_tail_wave(fa.sv, (int)(blockIdx.x - fa.n_prob), (int)(gridDim.x - fa.n_prob));
        return;
    }
    // distinct-task step: the problems of tasks >= *n_act are not evaluated (gp_reg_kernel)
    if (const int32_t* n_act = gpreg::KernelCtx{}.late(a.n_act, (unsigned)__builtin_offsetof(GpMfmaArgs, n_act))) {
        if (blockIdx.x >= (unsigned)*n_act * (unsigned)a.P) return;
    }
    constexpr int NB = 4, FP = 2, NP = 16 * NB, NU = NB * (NB + 1) / 2;      // the LDS of gp_reg_kernel<4, 2, true, false>, array by array
    __shared__ __attribute__((aligned(16))) float zf[NP * FP];
    __shared__ __attribute__((aligned(16))) float rv[NP];
    __shared__ __attribute__((aligned(16))) float av[NP];
    __shared__ __attribute__((aligned(16))) float fsc[gpreg::GPR_SCR];
    float* tsc = fsc;
    __shared__ __attribute__((aligned(16))) float dzc[NP * FP];
    __shared__ __attribute__((aligned(16))) float Wl[(NU - NB) * 256];
    {
        const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
        const unsigned t = blockIdx.x / (unsigned)a.P, p = blockIdx.x - t * (unsigned)a.P;
        const float* xt = fa.x + (long)t * NP * fa.d_in;
        float bx[4];
#pragma unroll
        for (int pb = 0; pb < 4; ++pb) bx[pb] = g < fa.d_in ? xt[(pb * 16 + r) * fa.d_in + g] : 0.0f;
        const float* th = fa.theta + (long)p * fa.theta_stride;
        const long blk0 = (long)p * fa.nblk + 4 * t;
        gpreg::fwd_net<NH, W32, true>(th + fa.off_mean, fa, 1, bx, fa.stash_mean, blk0, lane, zf, rv);
        asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0);
        gpreg::fwd_net<NH, W32, false>(th + fa.off_kern, fa, a.f, bx, fa.stash_kern, blk0, lane, zf, rv);
        asm volatile("" ::: "memory"); __builtin_amdgcn_wave_barrier();      // (one wave, in-order LDS: the body's lane i reads row i)
    }
    gpreg::gp_reg_body<NB, FP, true, false>(a, gpreg::FwdCtx{}, zf, rv, av, fsc, tsc, dzc, Wl);
}

// host only: does the fused launch cover this step?  fp32, RBF without outputscale, f <= 2, one 64-point task per stash tile, both
// networks on the fused MLP kernels (whose backward reads the stash) with 1-2 hidden layers, inputs shared by a task's P problems,
// a mean vector
static bool fwd_gp_applicable(int B, int P, int n, int x_div, int d_in, const int32_t* hidden, int n_hidden, int f_arg, int has_os,
                              int mean_mode, int dtype) {
    if (dtype != PACOH_F32 || kernel_of(f_arg) != PACOH_KERNEL_RBF || has_os || mean_mode != PACOH_MEAN_VECTOR) return false;
    const int f = features_of(f_arg);
    if (f < 1 || f > 2 || n != 64 || P <= 0 || B <= 0 || B % P != 0 || x_div != P || d_in < 1 || d_in > 4) return false;
    if (n_hidden < 1 || n_hidden > 2 || !hidden || g_sw.mlp_path != 0) return false;
    for (int l = 0; l < n_hidden; ++l) if (hidden[l] < 1 || hidden[l] > 32) return false;
    return (long)B * n <= 0x3fffffffL;
}

}  // namespace pacoh

using namespace pacoh;

extern "C" int pacoh_fwd_gp_applicable(int B, int P, int n, int x_div, int d_in, const int32_t* hidden, int n_hidden, int f,
                                       int has_outputscale, int mean_mode, int dtype) {
    return fwd_gp_applicable(B, P, n, x_div, d_in, hidden, n_hidden, f, has_outputscale, mean_mode, dtype) ? 1 : 0;
}

extern "C" int pacoh_fwd_gp_lml_fwdbwd(const pacoh_active_tasks* act, const void* x, int x_div, const void* theta, long theta_stride, int P,
                                       int d_in, const int32_t* hidden, int n_hidden, long off_mean, long off_kernel, void* stash,
                                       const void* svgd_X, void* svgd_workspace, int svgd_P, int svgd_D, int64_t* counter,
                                       const void* y, int y_div, const void* lengthscale, const void* outputscale, const void* noise,
                                       const int32_t* n_valid, const void* g_lml, void* lml, void* d_z, void* d_mean,
                                       void* d_lengthscale, void* d_outputscale, void* d_noise, int32_t* info,
                                       int B, int n, int f, int dtype, void* stream) {
    if (check_dtype(dtype)) return PACOH_EDTYPE;
    if (!x || !theta || !y || !lengthscale || !noise || !lml || !d_lengthscale || !d_noise || y_div <= 0 || off_mean < 0 || off_kernel < 0)
        return PACOH_EINVAL;
    if (act && (!act->n_act || !act->task_w)) return PACOH_EINVAL;
    if (svgd_X && (!svgd_workspace || svgd_P <= 0 || svgd_D <= 0)) return PACOH_EINVAL;
    if (svgd_X && svgd_P > PACOH_SVGD_MAX_PARTICLES) return PACOH_ELIMIT;
    if (!fwd_gp_applicable(B, P, n, x_div, d_in, hidden, n_hidden, f, outputscale != nullptr || d_outputscale != nullptr,
                           PACOH_MEAN_VECTOR, dtype))
        return PACOH_ELIMIT;
    GpMfmaArgs a = {nullptr, 1, nullptr, PACOH_MEAN_VECTOR, (const float*)y, y_div, (const float*)lengthscale, nullptr, (const float*)noise,
                    n_valid, (const float*)g_lml, (float*)lml, info, (float*)d_z, (float*)d_mean, (float*)d_lengthscale, nullptr,
                    (float*)d_noise, B, P, n, features_of(f)};
    if (act) { a.n_act = act->n_act; a.task_w = (const float*)act->task_w; }
    FwdGpArgs fa = {};
    fa.x = (const float*)x; fa.theta = (const float*)theta; fa.theta_stride = theta_stride;
    fa.off_mean = off_mean; fa.off_kern = off_kernel;
    fa.d_in = d_in; fa.h0 = hidden[0]; fa.h1 = n_hidden > 1 ? hidden[1] : 0;
    fa.nblk = 4 * (B / P);                                 // (mlp_fused.hip, fused_nblk at n = 64)
    if (stash && n_hidden > 1) {                           // (fused_n_stash: all hidden layers but the first; the two networks back to back)
        fa.stash_mean = (float*)stash;
        fa.stash_kern = (float*)stash + (size_t)P * fa.nblk * 2 * 256;
    }
    fa.n_prob = (unsigned)B;
    unsigned tail_wgs = 0;
    if (svgd_X) {
        float* d2 = (float*)svgd_workspace;
        fa.sv = SvgdDistTail<float>{(const float*)svgd_X, d2, d2 + svgd_P * svgd_P, svgd_P, svgd_D, (long*)counter};
        tail_wgs = (unsigned)(svgd_P * svgd_P);           // one particle pair each (the pairs j > i return at once)
    }
    const bool w32 = hidden[0] == 32 && (n_hidden == 1 || hidden[1] == 32);
    const dim3 grid((unsigned)B + tail_wgs);
    hipStream_t s = (hipStream_t)stream;
    if (n_hidden == 2) {
        if (w32) hipLaunchKernelGGL((gp_fwd_reg_kernel<2, true>), grid, dim3(64), 0, s, a, fa);
        else hipLaunchKernelGGL((gp_fwd_reg_kernel<2, false>), grid, dim3(64), 0, s, a, fa);
    } else {
        if (w32) hipLaunchKernelGGL((gp_fwd_reg_kernel<1, true>), grid, dim3(64), 0, s, a, fa);
        else hipLaunchKernelGGL((gp_fwd_reg_kernel<1, false>), grid, dim3(64), 0, s, a, fa);
    }
    return launch_status();
}

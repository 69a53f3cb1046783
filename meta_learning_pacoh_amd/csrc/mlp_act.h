// The tanh of the fused per-particle MLP kernels, shared by every kernel that runs their forward arithmetic (mlp_fused.hip,
// gp_fwd_reg.hip): one definition, so that the same activations come out bit for bit wherever they are computed.
#pragma once

namespace pacoh {

// tanh(y) = 1 - 2 / (1 + exp2(TSC y)), TSC = 2 log2(e).  The weights and biases of every tanh layer are multiplied by TSC when
// they are copied to LDS, so the matrix cores deliver the exp2 argument itself and an activation costs v_exp + v_add + v_rcp +
// v_fma (one instruction less, on each of the 64 activations per lane, tile and pass).  The backward pass multiplies by the
// SCALED hidden weights in its delta recursion, so delta_l comes out as TSC^(NH - l) times the true one (l = 1..NH): the
// accumulated weight gradients are scaled back once, where the slab is written.
constexpr float TSC = 2.8853900817779268f, INV_TSC = 0.34657359027997264f;
__device__ __forceinline__ float tanh_pre(float a) {
    return fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(a)), 1.0f);
}

}  // namespace pacoh

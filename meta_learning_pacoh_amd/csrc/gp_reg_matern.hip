// gp_reg_kernel / gp_reg_predict_kernel for the Matern families (PACOH_KERNEL_MATERN12 / 32 / 52): the register-resident fused
// task-GP kernel of gp_reg.hip on the same body (gp_reg_body.h), instantiated with the family's entry functions (RegFam, reg_kv,
// reg_kvd).  A file of its own so that gp_reg.hip's RBF kernels and their compile stay as they are, and the two build in parallel.
// fp32, n <= 128, f <= 4; every other shape of these families runs on the general kernels (gp_small.hip, dense_gp.hip).
// Reference: gpytorch.kernels.MaternKernel handed to the learners as covar_module (GPR_mll.py:41, GPR_meta_mll.py:42,224-225).
#include "gp_reg_body.h"

namespace pacoh {
namespace matern {

// waves per SIMD the register allocation aims at: gp_reg.hip's targets (GPR_MINW there), one wave fewer where the Matern kernel would
// spill at that target (tools/kernel_resources.sh: no Matern instantiation uses scratch).  The RBF kernels at these shapes spill a few
// registers themselves (8 - 152 bytes); the Matern body carries kv and kd of an entry and a longer chain per entry (sqrt, exp2, polynomial).
#define GPRM_MINW(NB, FP, BWD) ((NB) > 4 ? ((FP) == 2 || (NB) == 6 ? ((BWD) && (FP) == 4 ? 1 : 2) : 1) \
                                         : ((NB) == 4 && (FP) == 4 ? ((BWD) ? 2 : 3) : ((BWD) && (((NB) == 3 && (FP) == 4) || ((NB) == 4 && (FP) == 2)) ? 3 : 4)))
#define GPRM_PRED_MINW(NB, FP) ((NB) > 4 ? ((NB) == 6 && (FP) == 2 ? 2 : 1) : ((NB) == 4 ? ((FP) == 4 ? 2 : 3) : ((NB) == 3 && (FP) == 4 ? 3 : 4)))
template <int FAM, int NB, int FP, bool BWD>
__global__ void __launch_bounds__(64, GPRM_MINW(NB, FP, BWD)) gp_reg_kernel(GpMfmaArgs a) {
    constexpr int NP = 16 * NB;
    constexpr int NU = NB * (NB + 1) / 2;
    __shared__ __attribute__((aligned(16))) float zf[NP * FP];      // features * SC / lengthscale
    __shared__ __attribute__((aligned(16))) float rv[NP];           // residual
    __shared__ __attribute__((aligned(16))) float av[NP];           // alpha
    __shared__ __attribute__((aligned(16))) float fsc[gpreg::GPR_SCR];     // factor16() scratch = the transpose scratch (gp_reg.hip)
    float* tsc = fsc;
    __shared__ __attribute__((aligned(16))) float dzc[BWD ? NP * FP : 1];   // d_z before the chain-rule factors
    __shared__ __attribute__((aligned(16))) float Wl[BWD && NB > 1 && NB <= 4 ? (NU - NB) * 256 : 4];   // parked blocks of K^-1 (n <= 64)
    gpreg::gp_reg_body<NB, FP, BWD, true, gpreg::KernelCtx, false, FAM>(a, gpreg::KernelCtx{}, zf, rv, av, fsc, tsc, dzc, Wl);
}

template <int FAM, int NB, int FP>
__global__ void __launch_bounds__(64, GPRM_PRED_MINW(NB, FP)) gp_reg_predict_kernel(GpMfmaArgs a, GpPredArgs pa) {
    constexpr int NP = 16 * NB;
    __shared__ __attribute__((aligned(16))) float zf[NP * FP];
    __shared__ __attribute__((aligned(16))) float rv[NP];
    __shared__ __attribute__((aligned(16))) float av[NP];
    __shared__ __attribute__((aligned(16))) float fsc[gpreg::GPR_SCR];
    float* tsc = fsc;
    __shared__ __attribute__((aligned(16))) float dzc[4];
    __shared__ __attribute__((aligned(16))) float Wl[4];
    gpreg::gp_reg_body<NB, FP, true, true, gpreg::KernelCtx, true, FAM>(a, gpreg::KernelCtx{}, zf, rv, av, fsc, tsc, dzc, Wl, &pa);
}

template <int FAM, int NB>
static int launch_fam(const GpMfmaArgs& a, const GpPredArgs* pa, bool bwd, int FP, hipStream_t s) {
    if (pa) {
        if (FP == 2) hipLaunchKernelGGL((gp_reg_predict_kernel<FAM, NB, 2>), dim3((unsigned)a.B), dim3(64), 0, s, a, *pa);
        else hipLaunchKernelGGL((gp_reg_predict_kernel<FAM, NB, 4>), dim3((unsigned)a.B), dim3(64), 0, s, a, *pa);
    } else if (bwd) {
        if (FP == 2) hipLaunchKernelGGL((gp_reg_kernel<FAM, NB, 2, true>), dim3((unsigned)a.B), dim3(64), 0, s, a);
        else hipLaunchKernelGGL((gp_reg_kernel<FAM, NB, 4, true>), dim3((unsigned)a.B), dim3(64), 0, s, a);
    } else {
        if (FP == 2) hipLaunchKernelGGL((gp_reg_kernel<FAM, NB, 2, false>), dim3((unsigned)a.B), dim3(64), 0, s, a);
        else hipLaunchKernelGGL((gp_reg_kernel<FAM, NB, 4, false>), dim3((unsigned)a.B), dim3(64), 0, s, a);
    }
    return launch_status();
}

template <int NB>
static int launch_nb(const GpMfmaArgs& a, const GpPredArgs* pa, int kind, bool bwd, int FP, hipStream_t s) {
    switch (kind) {
        case PACOH_KERNEL_MATERN12: return launch_fam<PACOH_KERNEL_MATERN12, NB>(a, pa, bwd, FP, s);
        case PACOH_KERNEL_MATERN32: return launch_fam<PACOH_KERNEL_MATERN32, NB>(a, pa, bwd, FP, s);
        default: return launch_fam<PACOH_KERNEL_MATERN52, NB>(a, pa, bwd, FP, s);
    }
}

// pa != nullptr: the predictive (mu / var, V_out), otherwise the LML (+ gradients if bwd); returns 1 if this path does not apply
static int try_launch(const GpMfmaArgs& a, const GpPredArgs* pa, int kind, bool bwd, hipStream_t s) {
    if (!family_matern(kind) || a.n > 128 || a.f > 4 || a.n < 1 || a.f < 1 || (pa && pa->m < 1)) return 1;
    const int NB = (a.n + 15) / 16;
    const int FP = a.f <= 2 ? 2 : 4;
    switch (NB) {                                        // (5 and 7 blocks run on the 6- and 8-block kernels, as in gp_reg.hip)
        case 1: return launch_nb<1>(a, pa, kind, bwd, FP, s);
        case 2: return launch_nb<2>(a, pa, kind, bwd, FP, s);
        case 3: return launch_nb<3>(a, pa, kind, bwd, FP, s);
        case 4: return launch_nb<4>(a, pa, kind, bwd, FP, s);
        case 5: case 6: return launch_nb<6>(a, pa, kind, bwd, FP, s);
        default: return launch_nb<8>(a, pa, kind, bwd, FP, s);
    }
}

}  // namespace matern

int gp_reg_matern_try(const GpMfmaArgs& a, int kind, bool bwd, hipStream_t s) { return matern::try_launch(a, nullptr, kind, bwd, s); }
int gp_reg_matern_predict_try(const GpMfmaArgs& a, const GpPredArgs& pa, int kind, hipStream_t s) {
    return matern::try_launch(a, &pa, kind, true, s);
}

}  // namespace pacoh

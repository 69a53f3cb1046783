// Every PACOH_* environment switch the library honours, read ONCE when the library is loaded -- no getenv on
// a launch path.  Each one forces a path that a test covers; a host that changes the environment afterwards (the
// path-forcing tests, tools/mlp_time.py) calls pacoh_reload_env(), which reads it again.  Defined in misc.hip.
#pragma once

namespace pacoh {

struct Switches {
    // large-context (HBM-resident) path
    bool chol_ll, trtri_blocked, chol_blocked;
    bool gp8;                  // PACOH_GP8=0: the task-fused / persistent kernels run contexts of <= 8 points on the block body too (A/B, tests)
    int mlp_path;              // 0 fused, 1 mfma, 3 layers: the first implementation the dispatcher may pick
    int mt_nt;                 // PACOH_MT_NT=512 | 1024: threads per workgroup of the task-fused kernels (A/B; anything else: by the number of weight tiles)
};

extern Switches g_sw;
void read_switches(Switches& s);

}  // namespace pacoh

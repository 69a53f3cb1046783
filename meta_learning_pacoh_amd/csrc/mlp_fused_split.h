// The fused per-particle MLP kernels (mlp_fused.hip) when only the first *n_act tasks of a step's batch are live (the distinct tasks
// of a draw with replacement: include/pacoh_gp.h, pacoh_active_tasks).  The launch's grid was planned for all tb tasks -- `wgs`
// workgroups per (parameter row, network) of `tpw_host` tiles each, fixed for good once the step is captured in a graph -- so fewer
// rows do not shorten it unless the live tiles are dealt out again over the same workgroups, on the device:
//   * every tile live: the host's own count, whatever rounding produced it -- which rows meet in which workgroup's gradient slab
//     decides the bits of the sum, and a draw without repeats must give the bits of the plain call;
//   * fewer: an even share, rounded up to the four waves of a workgroup (a wave takes every fourth tile of its workgroup: the waves
//     of a workgroup then carry the same number of tiles, and the workgroups left over none at all), never more than the host's count.
// Workgroup w takes the tiles [w * tpw, (w + 1) * tpw) that lie below tiles_eff: they cover [0, tiles_eff) exactly once, since
// wgs * tpw >= tiles_eff either way.
#pragma once

namespace pacoh {

__host__ __device__ inline int fused_split_tiles(int tiles_eff, int tiles_full, int wgs, int tpw_host) {
    if (tiles_eff >= tiles_full) return tpw_host;
    const int share = ((tiles_eff + wgs - 1) / wgs + 3) & ~3;
    return share < tpw_host ? share : tpw_host;
}

}  // namespace pacoh

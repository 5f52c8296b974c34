// Launch planning for the MFMA fc kernels (linear_mfma.hip): the only copy of
// the tile and split rule, as plain integer arithmetic of the GEMM's sizes.
// No ATen and no HIP in here; bound to Python as `linear_mfma_plan`.
#pragma once

namespace fedkit_plan {

constexpr int kLinTile = 64;     // output tile edge and reduction tile depth
constexpr int kLinFill = 256;    // workgroups that fill the part (one per CU)
constexpr int kLinMaxSplits = 32;

struct LinearPlan {
  long long tiles_i;   // grid.x: ceil(I / 64)
  int tiles_j;         // grid.y: ceil(J / 64)
  int splits;          // grid.z: slices of the reduction axis (1 = no slab)
  int kt_per_split;    // reduction tiles per slice; every slice is non-empty
};

// out[I][J] = sum over R.  The reduction is cut until the grid reaches
// kLinFill workgroups, but never below two reduction tiles per workgroup
// (one tile leaves the double buffer nothing to overlap and doubles the slab
// traffic) and never into more than kLinMaxSplits slabs.  `splittable` is
// false for bwd-weight, whose reduction is the batch.
inline LinearPlan plan_linear(long long I, long long J, long long R,
                              bool splittable) {
  LinearPlan p{};
  p.tiles_i = (I + kLinTile - 1) / kLinTile;
  p.tiles_j = (int)((J + kLinTile - 1) / kLinTile);
  const long long nkt = (R + kLinTile - 1) / kLinTile;
  const long long tiles = p.tiles_i * p.tiles_j;
  long long per = nkt;
  if (splittable && tiles < kLinFill) {
    per = (nkt * tiles + kLinFill - 1) / kLinFill;
    if (per < 2) per = 2;
    const long long floor_per = (nkt + kLinMaxSplits - 1) / kLinMaxSplits;
    if (per < floor_per) per = floor_per;
    if (per > nkt) per = nkt;
  }
  // even slices: 8 tiles at 7 per slice are 2 slices of 4, not 7 + 1
  const long long splits = (nkt + per - 1) / per;
  per = (nkt + splits - 1) / splits;
  p.kt_per_split = (int)per;
  p.splits = (int)((nkt + per - 1) / per);
  return p;
}

}  // namespace fedkit_plan

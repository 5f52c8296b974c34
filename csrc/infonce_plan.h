// Launch planning for the tiled InfoNCE kernels (infonce_tiled.hip): the only
// copy of the tile and split rule of the similarity pass, as plain integer
// arithmetic of D and P.  No ATen and no HIP in here; bound to Python as
// `info_nce_tiled_plan`.
#pragma once

namespace fedkit_plan {

constexpr int kNceMinP = 64;      // at and below: the one-workgroup kernel
constexpr int kNceMaxP = 1024;    // above: the torch sequence
constexpr int kNceTile = 64;      // output tile edge of all three GEMMs
constexpr int kNceChunk = 32;     // reduction rows staged per step
constexpr int kNceFill = 512;     // workgroups wanted: two per CU
constexpr int kNceMaxSplits = 64;

struct InfoNcePlan {
  int tiles_p;            // ceil(P / 64): the similarity grid is tiles_p^2
  int splits;             // grid.z: slices of D (1 = one partial)
  int chunks_per_split;   // 32-row chunks per slice; every slice is non-empty
};

// zz[P][P] = sum over D.  D is cut until the grid reaches kNceFill
// workgroups, but never below two chunks per workgroup (one chunk leaves the
// double buffer nothing to overlap) and never into more than kNceMaxSplits
// partials (the row pass reads every one of them).
inline InfoNcePlan plan_info_nce(long long D, long long P) {
  InfoNcePlan p{};
  p.tiles_p = (int)((P + kNceTile - 1) / kNceTile);
  const long long tiles = (long long)p.tiles_p * p.tiles_p;
  const long long chunks = D < 1 ? 1 : (D + kNceChunk - 1) / kNceChunk;
  long long splits = 1;
  if (tiles < kNceFill) {
    splits = (kNceFill + tiles - 1) / tiles;
    if (splits > chunks / 2) splits = chunks / 2;
    if (splits > kNceMaxSplits) splits = kNceMaxSplits;
    if (splits < 1) splits = 1;
  }
  // even slices: 7 chunks in 3 slices are 3 + 3 + 1, never an empty slice
  const long long per = (chunks + splits - 1) / splits;
  p.chunks_per_split = (int)per;
  p.splits = (int)((chunks + per - 1) / per);
  return p;
}

}  // namespace fedkit_plan

// How a call is cut into work items and workgroups: host arithmetic only, shared by the launch
// path (gp_device.hip and the *_tu.hip launchers) and by gp_launch_plan, which reports it, so that the
// report cannot drift from the launch.  Every hot kernel is persistent: a launch takes
// min(cap, items) workgroups, cap = compute units x workgroups per CU, and a workgroup walks the
// items it is dealt (grid-stride, or a ticket counter in hessian_win_kernel).  One ROUND of a
// kernel is cap items = cap x rows_per_item test rows; beyond it workgroups run several items.
// The geometry constants stay with the kernels (Geo, WGeo, hk*, gk*, rk*): callers pass them in.
#pragma once

namespace gpk {

struct GridPlan {
  long long items;      // work items of the launch
  int workgroups;       // its grid
};

// Items = groups of rows_per_item rows, times the emulators of a batch (emulator-major); the grid is
// the persistent cap or the items, whichever is smaller.
inline GridPlan plan_grid(long long rows, int rows_per_item, long long n_emulators, long long cap) {
  GridPlan p;
  p.items = (rows + rows_per_item - 1) / rows_per_item * n_emulators;
  p.workgroups = (int)(p.items < cap ? p.items : cap);
  return p;
}

// predict: the few-rows kernel (a workgroup per 16-row tile) while every tile still gets a
// workgroup of its own within two rounds of the chip
inline bool plan_predict_few(long long tiles, int compute_units) { return tiles <= 2 * (long long)compute_units; }

// dynamic LDS of hessian_kernel: the training rows and [sqrt(e), centre]
inline unsigned long long hess_valu_lds_bytes(int elem_bytes, int nb, int row_stride, int kernel_d) {
  return (unsigned long long)elem_bytes * (16 * (unsigned long long)nb * row_stride + 2 * kernel_d);
}
// kernel dimensions that hessian_win_kernel is compiled for (where the matrix-core form beats or ties the VALU one)
inline bool hess_win_kernel_d(int kernel_d) {
  return kernel_d == 8 || kernel_d == 10 || kernel_d == 11 || kernel_d == 12 || kernel_d == 16;
}
// batched Hessian items are numbered in 32 bits, with room for the tickets drawn beyond the end
inline bool hess_items_fit(long long rows, int rows_per_item, long long n_emulators) {
  return (rows + rows_per_item - 1) / rows_per_item * n_emulators <= 0x7fffffffLL - 4 * 1024 * 1024;
}

// hessian_win_kernel, one call = at most two launches.  The LDSOUT instance (whole-line stores through
// LDS) takes the whole rows_per_item-row groups of the call when the kernel D has 16-byte rows
// (lds_out_d), the caller's rows are exactly D long and both pointers are 16-byte aligned; KL 3 when
// the instance without the last k-step exists for this block count (short_last) and the training set
// leaves that k-step empty.  What is left, and every other call, goes to the direct-store instance.
struct WinPlan {
  int ldsout_kl;        // 0: no LDSOUT launch; 3 or 4: its KL
  long long main_rows;  // rows of the LDSOUT launch (a multiple of rows_per_item)
  GridPlan main;
  long long rest_rows;  // rows of the direct-store launch (0: none)
  GridPlan rest;
};
inline WinPlan plan_hess_win(long long rows, int rows_per_item, int n_emulators, int cap, bool lds_out_d,
                             bool exact_d, bool aligned16, bool short_last, int n_ksteps, int kernel_nb) {
  WinPlan w = {0, 0, {0, 0}, rows, {0, 0}};
  const long long m_main = rows / rows_per_item * rows_per_item;
  if (lds_out_d && m_main > 0 && exact_d && aligned16) {
    w.ldsout_kl = short_last && n_ksteps == 4 * kernel_nb - 1 ? 3 : 4;
    w.main_rows = m_main;
    w.main = plan_grid(m_main, rows_per_item, n_emulators, cap);
    w.rest_rows = rows - m_main;
  }
  if (w.rest_rows > 0) w.rest = plan_grid(w.rest_rows, rows_per_item, n_emulators, cap);
  return w;
}

// reconstruct_kernel: the wide geometry (512 threads x 3 vectors) for band counts that one such
// workgroup covers whole and a narrow one (256 x 2) cannot; vec = elements per 16 bytes
inline bool recon_wide_default(int n_bands, int vec) { return n_bands > 256 * 2 * vec && n_bands <= 512 * 3 * vec; }
// items = 64-row tiles x band chunks of bands_per_wg; memory-bound, so a few workgroups per CU
// (cap), and every workgroup gets the same number of items (+-1): no workgroup is left with a
// whole extra round at the end
inline GridPlan plan_recon(long long n_rows, int rows_per_item, long long n_bands, long long bands_per_wg, long long cap) {
  GridPlan p;
  const long long chunks = (n_bands + bands_per_wg - 1) / bands_per_wg;
  p.items = (n_rows + rows_per_item - 1) / rows_per_item * chunks;
  const long long rounds = (p.items + cap - 1) / cap;
  p.workgroups = (int)((p.items + rounds - 1) / rounds);
  return p;
}
inline long long recon_cap(int compute_units, bool wide) { return (long long)compute_units * (wide ? 4 : 8); }

// misfit_kernel: items = groups of rows_per_item rows (a 16-row tile per wave, all bands); four 4-wave
// workgroups per CU (four waves per SIMD hide the observation stream), rounds balanced as above
inline long long misfit_cap(int compute_units) { return (long long)compute_units * 4; }
inline GridPlan plan_misfit(long long n_rows, int rows_per_item, long long cap) {
  GridPlan p;
  p.items = (n_rows + rows_per_item - 1) / rows_per_item;
  const long long rounds = (p.items + cap - 1) / cap;
  p.workgroups = (int)((p.items + rounds - 1) / rounds);
  return p;
}

// weight_gram_kernel: items and rounds as misfit_kernel's (plan_misfit).  The instance is the number of 16-pair
// blocks of the n_pcs (n_pcs + 1) / 2 pairs p <= q; its accumulators (8 reals per block and lane, 16 registers in
// fp64) decide how many 4-wave workgroups a CU holds, which is also what the kernel is compiled for.
constexpr int gram_blocks(int n_pcs) { return (n_pcs * (n_pcs + 1) / 2 + 15) / 16; }
constexpr int gram_wgs_per_cu(int blocks, int elem_bytes) {
  return elem_bytes == 8 ? (blocks <= 2 ? 4 : blocks <= 3 ? 3 : blocks <= 7 ? 2 : 1) : (blocks <= 4 ? 4 : blocks <= 7 ? 3 : 2);
}
inline long long gram_cap(int compute_units, int n_pcs, int elem_bytes) {
  return (long long)compute_units * gram_wgs_per_cu(gram_blocks(n_pcs), elem_bytes);
}

// lut_search_kernel: items = row tiles x slices of the candidate range (whole candidate tiles).  Row tiles alone
// fill the chip evenly only when they are several rounds of it: fewer are multiplied by slices, as many as fill one
// round (down to one candidate tile per slice) or, where the candidates allow, four rounds with at least four tiles
// per slice -- a single round of fewer items than the cap leaves some compute units one workgroup and others two.
// forced > 0: that many slices (tests), cut the same way.  Slices that would stay empty are not planned: n_slices is
// what the kernel is launched with.
struct LutPlan {
  long long row_tiles, cand_tiles, tiles_per_slice;
  int n_slices;
  GridPlan grid;
};
inline LutPlan plan_lut_search(long long n_rows, long long n_candidates, int rows_per_item, int cand_tile, long long cap,
                               int forced) {
  LutPlan p;
  p.row_tiles = (n_rows + rows_per_item - 1) / rows_per_item;
  p.cand_tiles = (n_candidates + cand_tile - 1) / cand_tile;
  long long s = forced;
  if (forced <= 0) {
    const long long one = (cap + p.row_tiles - 1) / p.row_tiles, four = (4 * cap + p.row_tiles - 1) / p.row_tiles;
    const long long s1 = one < p.cand_tiles ? one : p.cand_tiles;
    const long long s4 = four < p.cand_tiles / 4 ? four : p.cand_tiles / 4;
    s = s1 > s4 ? s1 : s4;
  }
  if (s > p.cand_tiles) s = p.cand_tiles;
  if (s < 1) s = 1;
  if (s > 0x7fff) s = 0x7fff;
  p.tiles_per_slice = (p.cand_tiles + s - 1) / s;
  p.n_slices = (int)((p.cand_tiles + p.tiles_per_slice - 1) / p.tiles_per_slice);
  p.grid.items = p.row_tiles * p.n_slices;
  p.grid.workgroups = (int)(p.grid.items < cap ? p.grid.items : cap);
  return p;
}
inline long long lut_cap(int compute_units, int wgs_per_cu) { return (long long)compute_units * wgs_per_cu; }

// lut_search_pc_kernel: lut_search_kernel's items, slices and persistent grid.  The instance is the padded n_pcs
// (8, 12 or 16: what its per-row registers are sized for); a lane holds the row's packed G, so the fp64 instances
// from 12 PCs on take more than 256 VGPRs and a CU holds one 4-wave workgroup of them, two of every other instance.
constexpr int lpMaxPcs = 16;         // the largest n_pcs the PC-space search and its set-up serve
constexpr int lut_pc_padded(int n_pcs) { return n_pcs <= 8 ? 8 : n_pcs <= 12 ? 12 : 16; }
constexpr int lut_pc_wgs_per_cu(int padded_pcs, int elem_bytes) { return elem_bytes == 8 && padded_pcs > 8 ? 1 : 2; }
inline LutPlan plan_lut_search_pc(long long n_rows, long long n_candidates, int rows_per_item, int cand_tile, long long cap,
                                  int forced) {
  return plan_lut_search(n_rows, n_candidates, rows_per_item, cand_tile, cap, forced);
}

// lut_posterior_kernel: lut_search_kernel's items and persistent grid, with the instance's own candidate tile.  The
// instance is the padded n_dims (8, 12 or 16: what the lane's 2 + DM + DM (DM + 1) / 2 double accumulators are sized
// for); every instance is built for one 4-wave workgroup per CU (the unified register file), and
// the instances of 16 dimensions take a 32-candidate tile.  The slices' partial sums -- n_rows x terms doubles per slice, far more
// than the search's lists -- stay within lqPartBytes of the context's scratch: the slices are capped by it, a forced
// count too, down to one slice, which needs no scratch at all.
constexpr int lqMaxDims = 16;
constexpr long long lqPartBytes = 256LL << 20;
constexpr int lut_post_padded(int n_dims) { return n_dims <= 8 ? 8 : n_dims <= 12 ? 12 : 16; }
constexpr int lut_post_tile(int padded_dims, int elem_bytes) { return elem_bytes == 8 || padded_dims > 8 ? 32 : 64; }
constexpr int lut_post_wgs_per_cu(int /*padded_dims*/, int /*elem_bytes*/) { return 1; }
__host__ __device__ constexpr long long lut_post_terms(int n_dims) { return 2 + n_dims + (long long)n_dims * (n_dims + 1) / 2; }
inline LutPlan plan_lut_posterior(long long n_rows, long long n_candidates, int n_dims, int rows_per_item, int cand_tile,
                                  long long cap, int forced) {
  LutPlan p = plan_lut_search(n_rows, n_candidates, rows_per_item, cand_tile, cap, forced);
  const long long room = lqPartBytes / (8 * lut_post_terms(n_dims) * n_rows);
  if (p.n_slices > 1 && p.n_slices > room) p = plan_lut_search(n_rows, n_candidates, rows_per_item, cand_tile, cap, room < 2 ? 1 : (int)room);
  return p;
}

// sobol_pair_kernel: items = (box, pair, block of skRows training rows), j-block fastest; plan_grid with the
// (box, pair) count as its batch.  The instance is the padded n_inputs (8, 12 or 16: what the per-lane registers are
// sized for); every instance takes more than 256 VGPRs, so a CU holds one 4-wave workgroup of it.
constexpr int skRows = 16, skThreads = 256;
constexpr int skMaxN = 512, skMaxD = 16;      // (a lane owns at most two columns; 16 D <= 256 threads form c^p)
constexpr int sobol_padded(int n_inputs) { return n_inputs <= 8 ? 8 : n_inputs <= 12 ? 12 : 16; }
constexpr int sobol_wgs_per_cu(int /*padded_inputs*/) { return 1; }
inline long long sobol_cap(int compute_units, int n_inputs) {
  return (long long)compute_units * sobol_wgs_per_cu(sobol_padded(n_inputs));
}
inline GridPlan plan_sobol(long long n_boxes, long long n_pairs, int n_train, long long cap) {
  return plan_grid(n_train, skRows, n_boxes * n_pairs, cap);
}

// sobol_inter_kernel: sobol_pair_kernel's items, limits and padded instances (plan_sobol).  The instances of 12 and 16
// inputs take more than 256 registers (DM (DM - 1) / 2 accumulators), so a CU holds one 4-wave workgroup of them; the
// instance of 8 takes 240 and is planned the same way (two a CU have not been measured).  A single input has no pair
// of inputs: nothing is launched.
constexpr int skInterWgsPerCu = 1;
inline long long sobol_inter_cap(int compute_units) { return (long long)compute_units * skInterWgsPerCu; }
inline GridPlan plan_sobol_inter(long long n_boxes, long long n_pairs, int n_train, int n_inputs, long long cap) {
  if (n_inputs < 2) return GridPlan{0, 0};
  return plan_sobol(n_boxes, n_pairs, n_train, cap);
}
// sobol_main_kernel: an item is one (box, emulator) over all inputs and grid points; 72 KB of LDS, two workgroups a CU
constexpr int smThreads = 256;
inline GridPlan plan_sobol_main(long long n_boxes, long long n_emulators, int compute_units) {
  return plan_grid(1, 1, n_boxes * n_emulators, 2LL * compute_units);
}

// moments_pair_kernel: an item is one (row, pair) over all n_train x n_train; plan_grid with one row per item.  The
// instance is the padded n_inputs (8, 12 or 16: the width of the g table in LDS, 512 x padded doubles, which with the
// other tables is 52, 69 and 85 KB of a CU's 160; two workgroups a CU where the registers allow it without spills).  The rows of a call run in slabs whose
// scratch -- (n_emulators + n_pairs)(n_inputs^2 + 1) doubles a row -- stays within gmSlabBytes.
constexpr int gmThreads = 256;
constexpr int gmMaxN = 512, gmMaxD = 16;      // (a lane owns at most two columns; an F is loaded by n_inputs^2 <= 256 threads)
constexpr long long gmSlabBytes = 256LL << 20;
constexpr int moments_padded(int n_inputs) { return n_inputs <= 8 ? 8 : n_inputs <= 12 ? 12 : 16; }
constexpr int moments_wgs_per_cu(int padded_inputs) { return padded_inputs <= 12 ? 2 : 1; }
inline long long moments_cap(int compute_units, int n_inputs) {
  return (long long)compute_units * moments_wgs_per_cu(moments_padded(n_inputs));
}
inline GridPlan plan_moments(long long n_rows, long long n_pairs, long long cap) { return plan_grid(n_rows, 1, n_pairs, cap); }
inline long long moments_slab_rows(long long n_rows, long long n_classes, int n_inputs) {
  const long long per_row = 8 * n_classes * ((long long)n_inputs * n_inputs + 1);
  const long long r = gmSlabBytes / per_row;
  return r < 1 ? 1 : r < n_rows ? r : n_rows;
}

}  // namespace gpk

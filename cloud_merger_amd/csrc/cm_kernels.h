// cm_kernels.h — launch wrappers of the gfx950 kernels (cm_kernels.hip), used by cm_launch.cpp (cmk_setup also by cm_api.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cm_device.h"

void cmk_setup(hipStream_t s, const CmFrameDev& f, CmFrameDev* d_frame, CmTileDev* d_tiles);   // d_tiles: cap_tiles entries, or nullptr
void cmk_minmax(hipStream_t s, const CmFrameDev* fd, float* partials, uint32_t n_blocks, const unsigned char* mask);
void cmk_keys(hipStream_t s, const CmFrameDev* fd, CmFrameState* st, uint32_t* keys, uint32_t* hist,
              uint32_t* grp_acc, uint32_t* grp_clear_a, uint32_t* grp_clear_b, uint32_t n_group_words,
              uint32_t n_clear_a_words, uint32_t* seg_groups, uint32_t n_seg_groups, const float* partials,
              uint32_t n_partials, int from_crop, int use_cell, const unsigned char* mask,
              const CmFrameState* st_outlier, uint32_t n_tiles);
// Outlier stage after the sort by the radius grid: gather into sorted order, row table, neighbour counts -> mask.
void cmk_outlier_mask(hipStream_t s, const CmFrameDev* fd, const CmFrameState* st, const uint32_t* keys_a,
                      const uint32_t* vals_a, const uint32_t* keys_b, const uint32_t* vals_b, void* sorted_pts,
                      void* rows, unsigned char* mask, uint32_t n_padded, const unsigned char* cls, uint32_t* pend_n,
                      bool already_gathered = false);
// ... its first half, which the statistical outlier stage shares: gather into sorted order (unless the bucket sort left the
// points gathered) and the (y,z)-row table.
void cmk_sorted_rows(hipStream_t s, const CmFrameDev* fd, const CmFrameState* st, const uint32_t* keys_a, const uint32_t* vals_a,
                     const uint32_t* keys_b, const uint32_t* vals_b, void* sorted_pts, void* rows, uint32_t n_padded,
                     bool already_gathered);
void cmk_hist(hipStream_t s, const CmFrameState* st, const uint32_t* keys, uint32_t* hist, uint32_t* grp,
              uint32_t pass, uint32_t n_tiles);
void cmk_gscan(hipStream_t s, const CmFrameState* st, uint32_t* grp, uint32_t* totals, uint32_t pass,
               uint32_t n_groups);
void cmk_scatter(hipStream_t s, CmFrameState* st, const uint32_t* keys_in, const uint32_t* vals_in,
                 uint32_t* keys_out, uint32_t* vals_out, const uint32_t* hist, const uint32_t* grp,
                 const uint32_t* totals, uint32_t pass, uint32_t n_tiles, uint32_t n_groups,
                 uint32_t n_padded, bool lds_rank, uint32_t* tile_kept = nullptr);
void cmk_probe_lds_order(hipStream_t s, uint32_t* violations, uint32_t rounds);
void cmk_seg_count(hipStream_t s, CmFrameState* st, const uint32_t* keys_a, const uint32_t* keys_b,
                   uint32_t* counts, uint32_t* group_counts, uint32_t min_pts, uint32_t n_seg_tiles);
// mode: 0 points -> centroids, 1 points -> partial entries, 2 partial entries -> merged entries
void cmk_seg_reduce(hipStream_t s, int mode, const CmFrameDev* fd, CmFrameState* st, CmFrameState* st_next,
                    uint32_t* host_state, const uint32_t* keys_a, const uint32_t* vals_a,
                    const uint32_t* keys_b, const uint32_t* vals_b, const uint32_t* counts,
                    const uint32_t* group_counts, void* out, uint32_t* out_key, uint32_t* out_cnt,
                    uint32_t n_seg_tiles);
void cmk_table_keys(hipStream_t s, const CmFrameDev* fd, CmFrameState* st, uint32_t* keys, uint32_t* hist,
                    uint32_t* grp_acc, uint32_t* grp_clear_a, uint32_t* grp_clear_b, uint32_t n_group_words,
                    uint32_t n_clear_a_words, uint32_t* seg_groups, uint32_t n_seg_groups, uint32_t key_bits,
                    uint32_t n_tiles);
void cmk_table_finish(hipStream_t s, const void* entries, uint32_t n, uint32_t min_pts, uint32_t* tile_counts,
                      uint32_t* total, void* out, uint32_t* out_key, uint32_t* out_cnt);
void cmk_to_pcl32(hipStream_t s, const void* in, void* out, uint32_t n);      // 16-byte records -> pcl::PointXYZI images
void cmk_merged(hipStream_t s, const CmFrameDev* fd, uint32_t* tile_counts, uint32_t* total, void* out,
                uint32_t n_tiles, const unsigned char* mask);

// ---- bucket path (cm_kernels_v2.hip) --------------------------------------------------------
// (f by value: the kernel reads the descriptor from its arguments; do_setup: it also leaves f in *fd and the tile table in tiles)
void cmk2_hist0(hipStream_t s, const CmFrameDev& f, CmFrameDev* fd, CmTileDev* tiles, bool do_setup, CmFrameState* st, uint32_t* hist, uint32_t* grp_acc,
                uint32_t* grp_clear_a, uint32_t* grp_clear_b, uint32_t n_group_words, uint32_t n_clear_a_words,
                unsigned long long* tile_state, uint32_t n_tile_state, float* records, int grid_mode, int check_box,
                uint32_t shift0, uint32_t n_global_passes, uint32_t n_tiles, const unsigned char* mask,
                const CmFrameState* st_outlier, int use_cell = 0, void* compact_out = nullptr, uint32_t* wave_cnt = nullptr);
void cmk2_hist(hipStream_t s, const CmFrameState* st, const unsigned char* dig, uint32_t* hist, uint32_t* grp,
               uint32_t n_tiles);                          // n_tiles: the grid (tiles of the records pass 0 kept: may be fewer than the frame's)
void cmk2_scatter(hipStream_t s, bool first, const CmFrameDev* fd, const CmTileDev* tiles, CmFrameState* st, const void* rec_in, void* rec_out,
                  unsigned char* dig_out, const uint32_t* hist, const uint32_t* grp, const uint32_t* totals,
                  uint32_t shift, uint32_t next_shift, uint32_t n_tiles, uint32_t n_groups, uint32_t n_padded,
                  const float* records, uint32_t n_records, int fold, const unsigned char* mask, int use_cell = 0,
                  const void* compact_in = nullptr, const uint32_t* wave_cnt = nullptr, int debug_swap = 0,
                  uint32_t* tile_kept = nullptr, bool sparse = false,    // sparse: k2_scatter_sparse (first pass over packed survivors)
                  bool ballot = false);                                  // ballot: ranks by ballots, not by returning LDS adds (cm_common.hpp)
void cmk2_local(hipStream_t s, const CmFrameDev* fd, CmFrameState* st, CmFrameState* st_next, uint32_t* host_state,
                const void* rec, unsigned long long* tile_state, uint32_t* ticket, void* out, uint32_t* out_key,
                uint32_t* out_cnt, void* partial_out, uint32_t low_bits, uint32_t n_padded);
// outlier stage: the records (x, y, z, padded index) fully sorted by radius-grid key, keys beside them
void cmk2_local_sort(hipStream_t s, const CmFrameDev* fd, CmFrameState* st, uint32_t* host_state, const void* rec,
                     uint32_t* keys_sorted, void* recs_sorted, uint32_t low_bits, uint32_t n_padded);

// ---- voxel finish of the bucket path, second generation (cm_kernels_v3.hip): k3_local + k3_compact
// tile_info: one uint2 per 2048-record tile; grp_cnt: one zeroed word per 64 tiles; stage: 16 B (32 B: partial) per record slot
// spl / bofs / n_buckets: the records are grouped by quantile bucket (cm_kernels_v4.hip): one workgroup per bucket;
// spl_next: where the finish leaves the next frame's splitters (CM4_MAX_BUCKETS + 1 words; nullptr: none)
void cmk3_local(hipStream_t s, const CmFrameDev* fd, CmFrameState* st, uint32_t* host_state, const void* rec, void* tile_info,
                uint32_t* grp_cnt, void* stage, uint32_t* stage_key, uint32_t* stage_cnt, bool partial, uint32_t low_bits,
                uint32_t n_slots,                          // n_slots / 2048 workgroups (n_padded, or what the records are expected to need)
                const uint32_t* spl = nullptr, const uint32_t* bofs = nullptr, uint32_t n_buckets = 0, uint32_t* spl_next = nullptr,
                bool ballot = false,
                uint32_t sub_shift = 0,                    // shared bins (cm_quant_sub_shift): bofs is per bin, 2^sub_shift buckets each,
                const unsigned char* dig = nullptr);       // dig[record] = the low sub_shift bits of its bucket number (cmk4_scatter)
void cmk3_local_big(hipStream_t s, const CmFrameDev* fd, CmFrameState* st, uint32_t* host_state, const void* rec, void* tile_info,
                    uint32_t* grp_cnt, void* stage, uint32_t* stage_key, uint32_t* stage_cnt, const uint32_t* spl, const uint32_t* bofs,
                    uint32_t n_buckets, uint32_t* spl_next, const uint32_t* big_list, bool ballot);
void cmk3_compact(hipStream_t s, const CmFrameState* st, CmFrameState* st_next, uint32_t* host_state, const void* tile_info,
                  const uint32_t* grp_cnt, const void* stage, const uint32_t* stage_key, const uint32_t* stage_cnt, void* out,
                  uint32_t* out_key, uint32_t* out_cnt, bool partial, uint32_t n_padded, uint32_t n_buckets = 0);

// ---- quantile passes (cm_kernels_v4.hip): one global pass into balanced buckets, then k3_local per bucket
// spl: CM4_MAX_BUCKETS + 1 splitters (ascending indices, spl[0] = 0, 0xFFFFFFFF beyond the frame's buckets); cnt: n_tiles rows of
// CM4_BINS 16-bit counters; totals: CM4_BINS words; bofs: CM4_BINS + 1 words (first record of every bucket, total)
void cmk4_hist(hipStream_t s, const CmFrameDev& f, CmFrameDev* fd, CmTileDev* tiles, bool do_setup, CmFrameState* st,
               const uint32_t* spl, uint32_t* cnt, uint16_t* bid, unsigned long long* tile_state, uint32_t n_tile_state, float* records,
               int grid_mode, int check_box, uint32_t n_tiles,        // bid: the bucket of every padded slot (0xFFFF: no record)
               uint32_t n_buckets,
               uint32_t* big_list,                                   // (word 0 zeroed: k4_colscan's list of buckets beyond CM4_CAP)
               uint32_t sub_shift,                                   // shared bins (cm_quant_sub_shift): counted per bucket >> sub_shift
               uint32_t* resident);                                  // three words of the context (0 at first): the grid-stride launch's size for 11, 12, 13 levels
// cap / cap_big / big_list: buckets of (cap, cap_big] records are listed (count, then numbers) for cmk3_local_big; beyond cap_big the frame aborts
void cmk4_colscan(hipStream_t s, CmFrameState* st, uint32_t* host_state, uint32_t* cnt, uint32_t* totals, uint32_t n_tiles,
                  uint32_t cap, uint32_t cap_big, uint32_t* big_list);
void cmk4_scatter(hipStream_t s, const CmFrameDev* fd, const CmTileDev* tiles, CmFrameState* st, const uint16_t* bid,
                  const uint32_t* cnt, const uint32_t* totals, uint32_t* bofs, uint32_t n_buckets, void* rec_out,
                  const float* records, uint32_t n_records, int fold, uint32_t* tile_kept, uint32_t n_tiles,
                  unsigned char* dig_out,                              // (shared bins: the low sub_shift bits of every record's bucket number)
                  bool ballot = false, const uint32_t* big_list = nullptr,    // (big_list: its count goes into CmFrameState.quant_big)
                  uint32_t sub_shift = 0);                             // shared bins: scattered by bucket >> sub_shift, dig_out = the low bits

// ---- zone-wise ground removal (cm_kernels_ground.hip) ------------------------------------------
void cmkg_setup(hipStream_t s, const CmGroundDev& g, CmGroundDev* d_ground);
// up to four byte arrays of n_bytes (a multiple of 16) set to a value each, up to two state records zeroed: one launch
void cmkg_clear(hipStream_t s, uint32_t n_bytes, void* p0, unsigned char v0, void* p1, unsigned char v1, void* p2, unsigned char v2,
                void* p3, unsigned char v3, CmFrameState* st_a, CmFrameState* st_b);
void cmkg_classify(hipStream_t s, const CmFrameDev* fd, const CmGroundDev* gd, CmFrameState* st, uint32_t* keys,
                   uint32_t* hist, uint32_t* grp_acc, uint32_t* grp_clear_a, uint32_t* grp_clear_b,
                   uint32_t n_group_words, uint32_t n_clear_a_words, unsigned char* keep_mask, unsigned char* zcode,
                   uint32_t n_tiles);
// slab offsets + band points in slab order, then one RANSAC workgroup per slab -> keep / ground masks
void cmkg_planes(hipStream_t s, const CmFrameDev* fd, const CmGroundDev* gd, const CmFrameState* st,
                 const uint32_t* keys_sorted, const uint32_t* vals_sorted, void* band_pts, uint32_t* zone_off,
                 void* hyp0, uint32_t* valid0, uint32_t* counts0, double* chunk_sums, CmGroundPlaneDev* planes,
                 unsigned char* keep_mask, unsigned char* ground_mask, uint32_t n_padded);

// ---- ego-motion compensation (cm_kernels_motion.hip) -------------------------------------------
// Every point of the frame's clouds (md: raw descriptors) transformed by its sensor's matrix and moved to the reference
// instant; written as 16-byte x,y,z,intensity records at the point's padded index into `out` (n_padded x 16 bytes).
void cmk_motion(hipStream_t s, const CmMotionDev& md, void* out, uint32_t n_padded);

// ---- per-voxel covariance of the last result (cm_kernels_cov.hip) --------------------------------
// recs / total: the frame's kept points as cmk_merged leaves them; keys: n_tiles * CM_TILE words; hist: n_tiles rows; grp: the
// pass-0 group rows (zeroed). Leaves in st what the radix kernels read (status, n_passes).
void cmk_cov_keys(hipStream_t s, const void* recs, const uint32_t* total, const CmCovGridDev& g, const uint32_t* out_key,
                  uint32_t n_out, uint32_t n_passes, CmFrameState* st, uint32_t* keys, uint32_t* hist, uint32_t* grp,
                  uint32_t n_tiles);
// One cm_voxel_cov per voxel into out (n_out x 80 B); a run that does not match out_cnt sets *err.
void cmk_cov_reduce(hipStream_t s, const void* recs, const CmFrameState* st_sort, const uint32_t* keys_a, const uint32_t* vals_a,
                    const uint32_t* keys_b, const uint32_t* vals_b, const uint32_t* out_cnt, uint32_t n_out, uint32_t min_points,
                    float eig_mult, void* out, uint32_t* err);

// ---- statistical outlier removal (cm_kernels_sor.hip) --------------------------------------------------------------------
// After cmk_sorted_rows on the stage's grid (st): the k-nearest-neighbour search (first: the 3x3x3 cells around every point;
// then the points it listed, ring by ring), the exact bins, the threshold, the keep-mask (points kept: 1).
void cmk_sor_knn(hipStream_t s, const CmFrameDev* fd, const CmFrameState* st, const uint32_t* keys_a, const uint32_t* keys_b,
                 const void* sorted_pts, const void* rows, float* dist, void* list, unsigned long long* words, uint32_t n_padded,
                 uint32_t k, bool first);
void cmk_sor_bins(hipStream_t s, const CmFrameState* st, const float* dist, unsigned long long* words, uint32_t n_padded);
void cmk_sor_threshold(hipStream_t s, const CmFrameState* st, unsigned long long* words, uint32_t k, float std_mul);
void cmk_sor_mask(hipStream_t s, const CmFrameState* st, const float* dist, unsigned long long* words, unsigned char* mask,
                  uint32_t n_padded);

// ---- Euclidean cluster extraction on the last result (cm_kernels_cluster.hip) ----------------------------------------------
// recs: the n result records. bounds: 6 words, [0..2] set to 0xFFFFFFFF and [3..5] to 0 before the launch.
void cmk_cl_bounds(hipStream_t s, const void* recs, uint32_t n, uint32_t* bounds);
// keys: n_tiles * CM_TILE words; hist: n_tiles rows; grp: the pass-0 group rows (zeroed). Leaves in st what the radix kernels
// and the row table read (status, n_passes, div_b).
void cmk_cl_keys(hipStream_t s, const void* recs, uint32_t n, const CmClusterGridDev& g, uint32_t n_passes, CmFrameState* st,
                 uint32_t* keys, uint32_t* hist, uint32_t* grp, uint32_t n_tiles);
// After the sort: pts = (x, y, z, result index) in sorted order; parent[i] = i; size / npts zeroed.
void cmk_cl_gather(hipStream_t s, const void* recs, const CmFrameState* st, const uint32_t* vals_a, const uint32_t* vals_b, uint32_t n,
                   void* pts, uint32_t* parent, uint32_t* size, uint32_t* npts);
// After cmk_sorted_rows on st's grid: every edge of the tolerance graph united in parent (indices of the result).
void cmk_cl_hook(hipStream_t s, const CmFrameState* st, const uint32_t* keys_a, const uint32_t* keys_b, const void* pts,
                 const void* rows, uint32_t n, float tol2, uint32_t* parent);
// root[i]; size[r] / npts[r] (sum of out_cnt; nullptr: left 0) at every root r.
void cmk_cl_roots(hipStream_t s, const uint32_t* parent, const uint32_t* out_cnt, uint32_t n, uint32_t* root, uint32_t* size,
                  uint32_t* npts);
// tile_sums: n_tiles uint2 -> exclusive (clusters, clustered voxels) before every tile; words[0] / [1]: the totals.
void cmk_cl_count(hipStream_t s, const uint32_t* root, const uint32_t* size, uint32_t n, uint32_t min_size, uint32_t max_size,
                  void* tile_sums, uint32_t* words, uint32_t n_tiles);
// num[i]: cluster number of a kept root, else CM_INVALID_KEY; clusters: first / n_voxels / n_points, empty AABB images.
void cmk_cl_number(hipStream_t s, const uint32_t* root, const uint32_t* size, const uint32_t* npts, const void* tile_excl,
                   uint32_t n, uint32_t min_size, uint32_t max_size, uint32_t* num, void* clusters, uint32_t n_tiles);
// labels[i]; the AABB images; keys / hist / grp / st for the sort of (cluster number, voxel index) as cmk_cl_keys leaves them.
void cmk_cl_labels(hipStream_t s, const void* recs, const uint32_t* root, const uint32_t* num, uint32_t n, uint32_t n_passes,
                   CmFrameState* st, uint32_t* labels, uint32_t* keys, uint32_t* hist, uint32_t* grp, void* clusters,
                   uint32_t n_tiles);
void cmk_cl_decode(hipStream_t s, void* clusters, uint32_t n_clusters);     // AABB images -> floats

// ---- normals and curvature of the last result (cm_kernels_normals.hip) ----------------------------------------------------
// After cmk_cl_gather and cmk_sorted_rows on st's grid g: the exact k nearest neighbours of every centroid by (d2, result
// index) and its entry (32 bytes at its result index in out). first: the 3x3x3 cells around each of the n centroids, the
// unfinished ones onto list (*list_n, zeroed before); then n_items = *list_n of them ring by ring. n_items 0: no launch.
void cmk_nrm_knn(hipStream_t s, const CmFrameState* st, const uint32_t* keys_a, const uint32_t* keys_b, const void* pts,
                 const void* rows, const void* recs, const CmClusterGridDev& g, uint32_t n, uint32_t k, const float viewpoint[3],
                 void* out, void* list, uint32_t* list_n, uint32_t n_items, bool first);

// ---- registration of a source cloud against the last result (cm_kernels_align.hip) -----------------------------------------
// After cmk_cl_gather and cmk_sorted_rows on st's grid g (cell >= 1.0039 r): one evaluation of `pose` over the n_src source
// records — the correspondences (8 bytes each, at the source index) and, per aligned block of 256, the 28 sums and the count
// (CM_ALIGN_STRIDE doubles per block). normals: the cm_voxel_normal table of the n_tgt result records recs. n_tgt 0: nothing
// is matched and st, the keys, pts, rows, recs and normals are not read. n_src 0: no launch.
void cmk_aln_eval(hipStream_t s, const CmFrameState* st, const uint32_t* keys_a, const uint32_t* keys_b, const void* pts,
                  const void* rows, const void* recs, const void* normals, const void* src, uint32_t n_src, uint32_t n_tgt,
                  const CmClusterGridDev& g, float r2, const CmAlignPoseDev& pose, void* corr, double* partials);
// sums[0..27]: the block partials added in ascending block order from 0.0; sums[28]: the count, a 64-bit integer.
void cmk_aln_sum(hipStream_t s, const double* partials, uint32_t n_blocks, double* sums);

// ---- NDT registration of a source cloud against the covariance table (cm_kernels_ndt.hip) -----------------------------------
// One evaluation of `pose` over the n_src source records against the n_out voxels whose sorted keys are out_key and whose
// cm_voxel_cov entries are cov, in the grid g (cmk_cov_keys'): the correspondences (16 bytes each, at the source index) and,
// per aligned block of 256, the 28 sums and the count in cmk_aln_eval's layout, for cmk_aln_sum. neighborhood: 1 or 7
// candidates per point; d2h: half of NDT's d2. n_out 0: out_key and cov are not read. n_src 0: no launch.
void cmk_ndt_eval(hipStream_t s, const uint32_t* out_key, uint32_t n_out, const void* cov, const void* src, uint32_t n_src,
                  const CmCovGridDev& g, uint32_t neighborhood, double d2h, const CmAlignPoseDev& pose, void* corr,
                  double* partials);

// ---- oriented boxes of the clusters (cm_kernels_box.hip) --------------------------------------------------------------------
// After the cluster call (clusters: its decoded table of n_clusters entries, indices: its member lists, recs: the result
// records): one cm_cluster_box per cluster into boxes. dirs: n_angles (cos, sin) pairs; step: the angle between two headings.
// A cluster of more than `split` members is listed instead of fitted: words[0] / [1] (zeroed before) count the listed
// clusters and their chunks, list / work / ext take one entry per listed cluster / chunk / (cluster, angle). The three
// launches behind it take the listed ones, with grids for the most there can be (max_chunks, max_large; 0: no launch);
// sums: n_angles doubles per listed chunk (cmk_box_sums is CLOSENESS's alone).
void cmk_box_fit(hipStream_t s, const void* recs, const void* clusters, const uint32_t* indices, uint32_t n_clusters,
                 const void* dirs, uint32_t n_angles, double step, uint32_t criterion, float d_min, uint32_t split, void* boxes,
                 uint32_t* words, void* list, void* work, void* ext);
void cmk_box_extremes(hipStream_t s, const void* recs, const void* clusters, const uint32_t* indices, const void* dirs,
                      uint32_t n_angles, const uint32_t* words, const void* list, const void* work, void* ext, uint32_t max_chunks);
void cmk_box_sums(hipStream_t s, const void* recs, const void* clusters, const uint32_t* indices, const void* dirs, uint32_t n_angles,
                  float d_min, const uint32_t* words, const void* list, const void* work, const void* ext, double* sums,
                  uint32_t max_chunks);
void cmk_box_choose(hipStream_t s, const void* clusters, const void* dirs, uint32_t n_angles, double step, uint32_t criterion,
                    const uint32_t* words, const void* list, const void* ext, const double* sums, void* boxes, uint32_t max_large);

// ---- 2-D grid map of the frame (cm_kernels_grid.hip) ------------------------------------------------------------------------
// table: nx * ny records of CM_GRID_WORDS words, zero bytes before cmk_grid_bin. cmk_grid_bin adds the frame's points (fd: the
// uploaded descriptor; keep: the frame's keep-mask or nullptr for "every valid point"; ground: its ground mask or nullptr for
// none) as images; cmk_grid_finish turns them into cm_grid_cell records in place and writes the occupancy bytes into image.
void cmk_grid_bin(hipStream_t s, const CmFrameDev* fd, const CmGridDev& g, const unsigned char* keep, const unsigned char* ground,
                  void* table, uint32_t n_tiles);
void cmk_grid_finish(hipStream_t s, void* table, void* image, uint32_t n_cells, float obstacle_height, uint32_t min_points);

// ---- free-space ray casting over the grid map (cm_kernels_rays.hip) ---------------------------------------------------------
// bits: per descriptor sensor a bitmap of `words` = ceil(nx * ny / 32) words, zero bytes before cmk_ray_mark, which sets the
// bit of every (sensor, cell) that holds a point cmk_grid_bin counts. rays: nx * ny records of (n_pass, n_end), zero bytes
// before cmk_ray_cast, which walks the set bits' rays from rd's origin cells. cmk_ray_finish writes the cleared bytes from
// the finished grid table (cmk_grid_finish's) and the ray table.
void cmk_ray_mark(hipStream_t s, const CmFrameDev* fd, const CmGridDev& g, const unsigned char* keep, const unsigned char* ground,
                  uint32_t* bits, uint32_t words, uint32_t n_tiles);
void cmk_ray_cast(hipStream_t s, const uint32_t* bits, uint32_t words, const CmRayDev& rd, uint32_t n_sensors, void* rays);
void cmk_ray_finish(hipStream_t s, const void* grid, const void* rays, void* image, uint32_t n_cells, uint32_t min_pass);

// ---- rolling log-odds occupancy map (cm_kernels_map.hip) ---------------------------------------------------------------------
// bits: 2 * n_sensors bitmaps of `words` = ceil(nx * ny / 32) words, zero bytes before cmk_map_mark: sensor s's E bitmap (the
// window cells of its counted points of A and G) at s * words — what cmk_ray_cast takes —, its H bitmap (of A alone) at
// (n_sensors + s) * words. cmk_map_update reads the old state (prev) at the shifted index, the ray table cmk_ray_cast left and
// the bitmaps, and writes the new state (next, another buffer) and the image.
void cmk_map_mark(hipStream_t s, const CmFrameDev* fd, const CmMapDev& g, const unsigned char* keep, const unsigned char* ground,
                  uint32_t* bits, uint32_t words, uint32_t n_sensors, uint32_t n_tiles);
void cmk_map_update(hipStream_t s, const void* prev, void* next, const void* rays, const uint32_t* bits, uint32_t words,
                    const CmMapUpdateDev& u, void* image);

// ---- cost layer over the occupancy map (cm_kernels_cost.hip) -------------------------------------------------------------------
// image: the map's three-valued image, ny rows of nx bytes. masks: ceil(ny / CM_COST_ROWS) * nx words, bit r of word
// (b, x) set iff cell (x, b * CM_COST_ROWS + r) is an obstacle (cmk_cost_colmask). carry: as many words, the nearest obstacle
// row of column x above block b in the low half and below it in the high half, CM_COST_NO_ROW where there is none
// (cmk_cost_colcarry). cmk_cost_rows writes dist2 (a word per cell) and cost (a byte per cell); lut holds g.r2 + 1 bytes.
// g.nx and g.ny are at most CM_COST_MAX_AXIS_DEV (a larger window is not launched).
void cmk_cost_colmask(hipStream_t s, const void* image, const CmCostDev& g, uint32_t* masks);
void cmk_cost_colcarry(hipStream_t s, const uint32_t* masks, const CmCostDev& g, uint32_t* carry);
void cmk_cost_rows(hipStream_t s, const void* image, const uint32_t* masks, const uint32_t* carry, const unsigned char* lut,
                   const CmCostDev& g, uint32_t* dist2, unsigned char* cost);

// ---- plan layer behind the cost layer (cm_kernels_plan.hip) ----------------------------------------------------------------------
// cost: the cost layer's table, ny rows of nx bytes. pot: a word per cell. flags: two tables of g.tiles_x * g.tiles_y words,
// one per tile, not zero: dirty. cmk_plan_init fills pot and both tables (the first is the first sweep's `cur`).
// cmk_plan_sweep relaxes the tiles that are dirty in cur, clears their words there, marks in next and adds the number of tiles
// that changed to *counter. cmk_plan_path walks from `start` and writes CM_PLAN_PATH_HEAD words and at most max_cells cells to out.
void cmk_plan_init(hipStream_t s, const CmPlanDev& g, uint32_t* pot, uint32_t* flags);
void cmk_plan_sweep(hipStream_t s, const unsigned char* cost, const CmPlanDev& g, uint32_t* pot, uint32_t* cur, uint32_t* next,
                    uint32_t* counter);
void cmk_plan_path(hipStream_t s, const unsigned char* cost, const uint32_t* pot, const CmPlanDev& g, uint32_t start, uint32_t max_cells,
                   uint32_t* out);

// ---- rollout layer behind the plan layer (cm_kernels_traj.hip) --------------------------------------------------------------------
// cost, pot: the cost and the plan layer's tables. steps: g.nv step lengths s_i (fp32). dh: g.nw heading increments. dirs:
// CM_TRAJ_HEADINGS_DEV (cos, sin) pairs. foot: g.n_foot (bx, by) pairs. cmk_traj_roll writes g.nv * g.nw records, entry
// i * g.nw + j; cmk_traj_best reduces them to CM_TRAJ_INFO_WORDS words (best, n_valid).
void cmk_traj_roll(hipStream_t s, const unsigned char* cost, const uint32_t* pot, const CmTrajDev& g, const float* steps, const uint32_t* dh,
                   const float* dirs, const float* foot, CmTrajScoreDev* out);
void cmk_traj_best(hipStream_t s, const CmTrajScoreDev* scores, uint32_t n, uint32_t* info);

// ---- scan matching layer behind the cost layer (cm_kernels_match.hip) ---------------------------------------------------------------
// dist2: the cost layer's table. lut: the field table, r2 + 1 bytes. field: one byte per window cell. q: six floats per
// candidate (rows 0 and 1 of its linear part). bits: g.n_k bitmaps of g.words words, zero before cmk_match_mark. vol:
// g.n_k * (2 wy + 1) * (2 wx + 1) words, zero before cmk_match_score. cmk_match_best writes CM_MATCH_INFO_WORDS words.
void cmk_match_field(hipStream_t s, const uint32_t* dist2, const unsigned char* lut, uint32_t r2, uint32_t n_cells, unsigned char* field);
void cmk_match_mark(hipStream_t s, const CmFrameDev* fd, const CmMatchDev& g, const float* q, const unsigned char* keep, uint32_t* bits,
                    uint32_t n_tiles);
void cmk_match_score(hipStream_t s, const unsigned char* field, const uint32_t* bits, const CmMatchDev& g, uint32_t* vol);
void cmk_match_best(hipStream_t s, const uint32_t* vol, const uint32_t* bits, const CmMatchDev& g, uint32_t* info);

// ---- localisation layer behind the cost layer (cm_kernels_mcl.hip) -------------------------------------------------------------------
// parts: g.n particles; wts: g.n records; words: the CM_MCL_WORDS info words. bits: a bitmap of n_words words (the body bitmap,
// zero before cmk_mcl_mark, or the free-cell bitmap cmk_mcl_free_bits writes); counts: one word per CM_MCL_BLOCK bitmap words, at
// most CM_MCL_ONE_BLOCK of them. cmk_mcl_compact is the ordered compaction of a bitmap, three launches: the set bits in
// ascending order, every stride-th of them into list (at most max_out, the stride chosen on the device), their numbers into
// words[CM_MCL_W_NCELLS .. CM_MCL_W_NBEAMS]. cmk_mcl_score reads the beams from list and words. dirs: the heading table. cum: g.n
// 64-bit prefix sums. cmk_mcl_resample writes the decision into words and, where it falls, the new particles into dst;
// otherwise it sets src's parents. r_draw: splitmix64(base ^ 1 << 63). thr: resample_frac * n_particles, always: the flag.
void cmk_mcl_mark(hipStream_t s, const CmFrameDev* fd, const CmMclDev& g, const unsigned char* keep, uint32_t* bits, uint32_t n_tiles);
void cmk_mcl_free_bits(hipStream_t s, const void* image, uint32_t n_cells, uint32_t* bits);
void cmk_mcl_compact(hipStream_t s, const uint32_t* bits, uint32_t n_words, uint32_t max_out, uint32_t* counts, uint32_t* list,
                     unsigned long long* words);
void cmk_mcl_init_pose(hipStream_t s, const CmMclMoveDev& m, uint32_t n, CmMclParticleDev* parts);
void cmk_mcl_init_uniform(hipStream_t s, const CmMclDev& g, unsigned long long base, const uint32_t* list, const unsigned long long* words,
                          CmMclParticleDev* parts);
void cmk_mcl_predict(hipStream_t s, const CmMclMoveDev& m, uint32_t n, const float* dirs, CmMclParticleDev* parts);
void cmk_mcl_score(hipStream_t s, const unsigned char* field, const CmMclDev& g, const uint32_t* list, const unsigned long long* words,
                   const float* dirs, CmMclParticleDev* parts, CmMclWeightDev* wts);
// The beam model's score in cmk_mcl_score's place: image, the map's image; steps, the skip bytes cmk_cast_steps wrote (not read
// under bm.plain); table, the 2 * bm.over + 3 bytes of cm_mcl_beam_table on the device; counts, the CM_MCL_BEAM_COUNTS 64-bit
// outcome counts, zero before the launch.
void cmk_mcl_beam(hipStream_t s, const void* image, const unsigned char* steps, const unsigned char* table, const CmMclDev& g, const CmMclBeamDev& bm,
                  const uint32_t* list, const unsigned long long* words, const float* dirs, CmMclParticleDev* parts, CmMclWeightDev* wts,
                  unsigned long long* counts);
void cmk_mcl_best(hipStream_t s, const CmMclParticleDev* parts, uint32_t n, unsigned long long* words);
void cmk_mcl_weights(hipStream_t s, const CmMclParticleDev* parts, uint32_t n, double beta, const float* dirs, CmMclWeightDev* wts,
                     unsigned long long* words);
void cmk_mcl_spread(hipStream_t s, const CmMclParticleDev* parts, uint32_t n, const CmMclWeightDev* wts, unsigned long long* words);
// base: the update's draw base; hy: the hypotheses mode (hy.on == 0: off, the step is the layer's own step 10).
void cmk_mcl_resample(hipStream_t s, CmMclParticleDev* src, CmMclParticleDev* dst, const CmMclDev& g, const CmMclWeightDev* wts, unsigned long long* cum,
                      unsigned long long base, unsigned long long r_draw, double thr, uint32_t always, unsigned long long* words, const CmMclHypDev& hy);
// The hypotheses mode (CmMclHypDev, cm_device.h), between cmk_mcl_spread and cmk_mcl_resample, over the particles and the
// weights of the update. Before cmk_mcl_hyp_bins: hy.keys all CM_MCL_HYP_EMPTY and hy.words[0 .. CM_MCL_HW_CLEARED) zero. With
// hy.inject_max > 0 the free cells' compaction goes into hy.words and hy.free_list before cmk_mcl_hyp_recover, which reads
// n_beams from the layer's words. cmk_mcl_hyp_flatten is two launches: the roots' numbers, then every slot's.
void cmk_mcl_hyp_bins(hipStream_t s, const CmMclParticleDev* parts, const CmMclHypDev& hy);
void cmk_mcl_hyp_link(hipStream_t s, const CmMclHypDev& hy);
void cmk_mcl_hyp_flatten(hipStream_t s, const CmMclHypDev& hy);
void cmk_mcl_hyp_sums(hipStream_t s, const CmMclParticleDev* parts, const CmMclWeightDev* wts, const float* dirs, const CmMclHypDev& hy);
void cmk_mcl_hyp_spread(hipStream_t s, const CmMclParticleDev* parts, const CmMclWeightDev* wts, const CmMclHypDev& hy);
void cmk_mcl_hyp_pick(hipStream_t s, const CmMclHypDev& hy);
void cmk_mcl_hyp_recover(hipStream_t s, const CmMclHypDev& hy, const unsigned long long* layer_words);
// The image of a state table (the map's step 8), for cm_map_load: (logodds, n_obs) per cell into one byte per cell.
void cmk_map_image(hipStream_t s, const void* state, uint32_t n_cells, int l_free, int l_occ, void* image);

// ---- cast layer behind the cost layer (cm_kernels_cast.hip) ---------------------------------------------------------------------------
// steps: one byte per window cell, cmk_cast_steps writes it from dist2 (the skip table; not read under g.plain). poses: g.n_poses
// records g.pose_words words apart, x, y and h in the first three. bearings: g.n_bearings binary angles. dirs: CM_CAST_DIRS pairs of
// int16_t. rays: g.n_poses * g.n_bearings records of cm_cast_ray. words: the CM_CAST_WORDS status counts, zero before the launch.
void cmk_cast_steps(hipStream_t s, const uint32_t* dist2, uint32_t n_cells, unsigned char* steps);
void cmk_cast_rays(hipStream_t s, const void* image, const unsigned char* steps, const CmCastDev& g, const void* poses, const uint32_t* bearings,
                   const void* dirs, void* rays, uint32_t* words);

// ---- frontier layer behind the plan layer (cm_kernels_front.hip) -------------------------------------------------------------------
// image, cost, pot: the map's image, the cost and the plan layer's tables. labels: a word per cell (parents, then roots, then
// frontier numbers). size: a word per cell (a root's cell count, then its number). counts: g.n_blocks words. info:
// CM_FRONT_INFO_WORDS words, zero before cmk_front_local. table: g.max_frontiers entries; box: four words per entry.
// The calls run in this order; every one is a single launch.
void cmk_front_local(hipStream_t s, const void* image, const unsigned char* cost, const CmFrontDev& g, uint32_t* labels, uint32_t* size,
                     uint32_t* info);
void cmk_front_merge(hipStream_t s, const CmFrontDev& g, uint32_t* labels);
void cmk_front_flatten(hipStream_t s, const CmFrontDev& g, uint32_t* labels, uint32_t* size);
void cmk_front_count(hipStream_t s, const CmFrontDev& g, const uint32_t* labels, const uint32_t* size, uint32_t* counts, uint32_t* info);
void cmk_front_scan(hipStream_t s, const CmFrontDev& g, uint32_t* counts, uint32_t* info);
void cmk_front_number(hipStream_t s, const CmFrontDev& g, const uint32_t* labels, uint32_t* size, const uint32_t* counts,
                      CmFrontEntryDev* table, uint32_t* box);
void cmk_front_table(hipStream_t s, const CmFrontDev& g, const uint32_t* pot, uint32_t* labels, const uint32_t* size,
                     CmFrontEntryDev* table, uint32_t* box);
void cmk_front_best(hipStream_t s, const CmFrontDev& g, CmFrontEntryDev* table, const uint32_t* box, uint32_t* info);

// ---- search layer behind the cost layer (cm_kernels_msearch.hip) ---------------------------------------------------------------------
// Level h of the pyramid is (ny + 2^h - 1) rows of (nx + 2^h - 1) bytes; cmk_msearch_pyramid makes level h >= 1 (dst) from
// level h - 1 (src). bits: the g.n_k bitmaps cmk_match_mark filled; cells: g.n_k lists of g.max_cells words; counts: g.n_k
// words, zero before cmk_msearch_list. list / n_ptr / n_max: nodes, their number in device memory, and the host's bound on
// it (the grid). U: one score per node of the list; with splits > 1 a node's cells are spread over that many workgroups, which
// add into U, zero before the launch. words: the CM_MSEARCH_WORDS info words. cmk_msearch_select adds the live
// nodes of the n-node list at level h >= 1 to counters[0] and their children to counters[1] and writes at most cap of them.
void cmk_msearch_pyramid(hipStream_t s, const unsigned char* src, unsigned char* dst, uint32_t nx, uint32_t ny, uint32_t h);
void cmk_msearch_list(hipStream_t s, const uint32_t* bits, const CmMSearchDev& g, uint32_t words, uint32_t* cells, uint32_t* counts);
void cmk_msearch_score(hipStream_t s, const uint32_t* list, const uint32_t* n_ptr, uint32_t n_max, const CmMSearchDev& g, const unsigned char* tab,
                       uint32_t h, const uint32_t* cells, const uint32_t* counts, uint32_t splits, uint32_t* U);
void cmk_msearch_pick(hipStream_t s, const uint32_t* list, const uint32_t* U, const uint32_t* n_ptr, uint32_t n_max, const CmMSearchDev& g, uint32_t h,
                      uint32_t* words);
void cmk_msearch_select(hipStream_t s, const uint32_t* list, const uint32_t* U, uint32_t n, const CmMSearchDev& g, uint32_t h, const uint32_t* bound,
                        uint32_t* next, uint32_t cap, uint32_t* counters);
void cmk_msearch_best(hipStream_t s, const uint32_t* list, const uint32_t* U, uint32_t n, const CmMSearchDev& g, const uint32_t* counts, uint32_t* words);

// ao_amd/csrc/internal.h -- the library's internal interface: every function that one .hip unit defines and another calls
// and that include/ptv2_hip.h does not declare, once, under the unit that defines it.  common.h includes it, so the defining
// unit sees the declaration too and the compiler checks the two against each other (an extern "C" symbol carries no
// signature: nothing else would).  Types taken by reference or value are only named here; the callers include what defines
// them: gva_common.h the attention operand bundles (AttnIn ... LogitsBwdOut, next to FoldWFwdArgs), dense_common.h
// BnTileSet, wgrad_job.h WgradJob.  (common.h and gva_common.h keep the interfaces that sit next to their types.)
#pragma once

struct GvaPlan;  // gva_plan.h
namespace gva {
struct FoldWFwdArgs; struct FoldWBwdArgs; struct PtvDrop;
struct AttnIn; struct AttnFwdOut; struct AttnBwdIn; struct AttnBwdOut;
struct LogitsIn; struct LogitsOut; struct LogitsBwdIn; struct LogitsBwdOut;
}
namespace dense { struct WgradJob; struct BnTileSet; }

// ---- abi.hip ----------------------------------------------------------------------------------------------------------
void ptv2_profile_scope(int which, int end, int ring_entry, int ring_size);
// ---- gemm.hip ---------------------------------------------------------------------------------------------------------
// rows per statistics / reduce record the fused row GEMMs write for a shape (16: the deep levels' k-split kernel),
// and the switch that tells them this caller reads either
int rows_gemm_record_rows(int m, int n, int k);
void ptv2_gemm_allow_rb16(int on);
// ---- bn.hip -----------------------------------------------------------------------------------------------------------
size_t bn_tiles_floats_rb(int n, int c, int rb);  // floats of a statistics record buffer with records of rb rows each
// a set names its record buffer (and the rows per record, S.rb), mean / rstd, running buffers, gamma / beta and sc / sh
int bn_tiles_finalize_rb(int n, int c, const dense::BnTileSet &S, float eps, float momentum, void *stream);
int bn_tiles_finalize_pair(int n, int c, const dense::BnTileSet (&S)[2], float eps, float momentum, void *stream);
int bn_tiles_apply_residual(int n, int c, const dense::BnTileSet &S, float eps, float momentum, const float *x,
                            const float *residual, const float *rowscale, float *y, void *stream);
int bn_tiles_apply_relu(int n, int c, const dense::BnTileSet &S, float eps, float momentum, const float *x, float *y, void *stream);
// ---- skinny.hip -------------------------------------------------------------------------------------------------------
int skinny_linear_forward_pair(int n, int cin, int cout, const float *const *x, const float *W, const float *const *xsc,
                               const float *const *xsh, float *const *y, void *stream);
// the q / k BatchNorms' reduce inside the skinny input-gradient launch: armed by block.hip, run by gva_block.hip, and the
// BatchNorm pair launcher (bn.hip) takes the count of records it left (0: none)
void ptv2_skinny_bn_arm(int n, int c, const float *const *x, const float *const *gy, const float *const *mean,
                        const float *const *rstd, const float *const *gamma, const float *const *beta, int relu, void *workspace,
                        size_t workspace_bytes);
void ptv2_skinny_bn_disarm(void);
struct PtvSkinnyBnScope {  // disarmed when the scope that may have armed it is left
    PtvSkinnyBnScope() = default;
    ~PtvSkinnyBnScope() { ptv2_skinny_bn_disarm(); }
    PtvSkinnyBnScope(const PtvSkinnyBnScope &) = delete;
    PtvSkinnyBnScope &operator=(const PtvSkinnyBnScope &) = delete;
};
int skinny_backward_pair_bn_reduce(int n, int cin, int cout, const float *const *gy, const float *W, float *const *gx,
                                   void *stream);
int ptv2_skinny_bn_take_records(int n, int c, const float *part, const float *const *gy);
// ---- wgrad.hip --------------------------------------------------------------------------------------------------------
// linear_wgrad_strided_hip_launcher with rowscale != NULL asking for db[b][o] = sum_n gY[n, b, o] * rowscale[n * lds_s + b]
// instead of the plain column sums.  Only the LDS-staged fp32 kernel forms them: *weighted says whether it did (1) or
// whether the caller has to compute db itself (0: db is then not written at all).
extern "C" int linear_wgrad_strided_rowscale(int n, int cout, int cin, int batch, const float *gY, long long ldy, long long sy,
                                             const float *X, long long ldx, long long sx, float *dW, float *db,
                                             const float *rowscale, long long lds_s, int *weighted, void *workspace,
                                             size_t workspace_bytes, void *stream);
int gva_wp2_wgrad_recompute(int n, int k, int c, int g, const gva::AttnIn &I, const gva::AttnBwdIn &X, float *dW, float *db,
                            void *workspace, size_t workspace_bytes, void *stream);
// ---- block.hip --------------------------------------------------------------------------------------------------------
int ptv2_blocks_fold_forward(int count, const ptv2_block *blocks, void *stream);
// ---- gva_block.hip ----------------------------------------------------------------------------------------------------
int gva_fold_forward_batched(int count, const ptv2_gva_block *blocks, void *stream);
int gva_block_forward_stats(const ptv2_gva_block *B, float *out_stats, int *stats_done, void *workspace, size_t workspace_bytes,
                            void *stream);
void ptv2_gva_set_prefolded(int on);
size_t ptv2_gva_fold_scratch_floats(int c, int g);  // deferred M / cW glue of the attention backward
void ptv2_gva_set_fold_scratch(float *p);
int ptv2_gva_flush_folds(void *stream);
void ptv2_gva_drop_folds();
// ---- gva_fwd.hip ------------------------------------------------------------------------------------------------------
int gva_logits_forward_fold(const GvaPlan &P, int n, int k, int c, int g, const gva::LogitsIn &I, const gva::LogitsOut &O,
                            const gva::FoldWFwdArgs &F, void *workspace, size_t workspace_bytes, void *stream);
// ---- gva_fwd_point.hip ------------------------------------------------------------------------------------------------
int gva_fwd_point_supported(int k, int c, int g);
int gva_fwd_point_max_n();
int gva_fwd_point_launch(int n, int k, int c, int g, const gva::AttnIn &I, const gva::AttnFwdOut &O, void *stream);
// ---- gva_fwd_tile.hip -------------------------------------------------------------------------------------------------
int gva_fwd_tile_supported(int k, int c, int g);
int gva_fwd_tile_launch(int n, int k, int c, int g, const gva::AttnIn &I, const gva::AttnFwdOut &O, void *stream);
// ---- gva_peb.hip ------------------------------------------------------------------------------------------------------
// reads O.A, O.sw, O.out_v; writes O.out, O.stats
int gva_peb_forward_stats(int n, int c, int g, const gva::AttnIn &I, const gva::AttnFwdOut &O, int *stats_done, void *stream);
// ---- gva_aggregate.hip ------------------------------------------------------------------------------------------------
// the public stage launchers behind a plan the caller has made already (gva_block.hip)
int gva_aggregate_forward(const GvaPlan &P, int n, int k, int c, int g, const gva::AttnIn &I, const gva::AttnFwdOut &O,
                          void *stream);
// X.g_A / X.g_sw, or NULL for both and I.Wp2 / I.bp2 where the plan says fused_peb
int gva_aggregate_backward(const GvaPlan &P, int n, int k, int c, int g, const gva::AttnIn &I, const gva::AttnBwdIn &X,
                           const gva::AttnBwdOut &O, void *workspace, size_t workspace_bytes, void *stream);
// ---- gva_bwd.hip ------------------------------------------------------------------------------------------------------
// F.gsc != NULL: gT1 / gT2 are not read; the rows kernel derives them from the fold_w backward (and writes the BatchNorm's
// parameter gradients)
int gva_logits_backward_foldw(const GvaPlan &P, int n, int k, int c, int g, const gva::LogitsIn &I, const gva::LogitsBwdIn &X,
                              const gva::FoldWBwdArgs &F, const gva::LogitsBwdOut &O, void *workspace, size_t workspace_bytes,
                              void *stream);
// ---- gva_bwd_logits.hip -----------------------------------------------------------------------------------------------
int gva_logits_bwd_fused_supported(int k, int c, int g);
int gva_logits_bwd_fused_launch(int n, int k, int c, int g, const gva::LogitsIn &I, const gva::LogitsBwdIn &X,
                                const gva::FoldWBwdArgs &F, float *gWt, float *part, size_t part_floats_avail,
                                const gva::LogitsBwdOut &O, hipStream_t st);
int gva_logits_fwd_mfma_supported(int k, int c, int g);
int gva_logits_fwd_mfma_launch(int n, int k, int c, int g, const gva::LogitsIn &I, const gva::LogitsOut &O, float *part,
                               const gva::FoldWFwdArgs &F, hipStream_t st);
// ---- gva_bwd_point.hip: the fused MFMA backward (one launch) for the (k, c, g) it is instantiated for -----------------
int gva_bwd_point_supported(int k, int c, int g);
int gva_bwd_point_local(int k, int c, int g);  // the instances that can form g_A / g_sw themselves (shape only; gva_plan() decides)
size_t gva_bwd_point_part_floats(int c, int g);
// part: the workgroup records (part_floats_avail floats), summed into O.gsc ... O.gb by the finalize
int gva_bwd_point_launch(int n, int k, int c, int g, const gva::AttnIn &I, const gva::AttnBwdIn &X, const gva::AttnBwdOut &O,
                         float *part, size_t part_floats_avail, hipStream_t st, gva::PtvDrop drop);
int gva_softmax_point_launch(int n, int k, int g, const gva::AttnIn &I, const gva::AttnFwdOut &O, hipStream_t st,
                             gva::PtvDrop drop);
int gva_logits_point_launch(int n, int k, int c, int g, const gva::LogitsIn &I, const gva::LogitsOut &O, float *part,
                            const gva::FoldWFwdArgs &F, hipStream_t st);
int gva_logits_params_point_launch(int n, int k, int c, int g, const gva::LogitsIn &I, const float *gWt, float *part,
                                   int max_blocks, int *nblk_out, hipStream_t st);
// ---- gva_bwd_tile.hip: the deep levels' backward per tile of points, g_A formed in the kernel -------------------------
int gva_bwd_tile_supported(int k, int c, int g);
size_t gva_bwd_tile_part_floats(int n, int c, int g);
int gva_bwd_tile_launch(int n, int k, int c, int g, const gva::AttnIn &I, const gva::AttnBwdIn &X, const gva::AttnBwdOut &O,
                        float *part, size_t part_floats_avail, gva::PtvDrop drop, hipStream_t st);
// ---- gva_wgrad_tile.hip -----------------------------------------------------------------------------------------------
int gva_wgrad_tile_supported(int k, int c, int g);
size_t gva_wgrad_tile_plan(dense::WgradJob *J, int max_splits);
int gva_wgrad_tile_launch_one(const dense::WgradJob &J, hipStream_t st);
int gva_wgrad_tile_launch_jobs(const dense::WgradJob *table, int njobs, int wgs, int pos_wgs, hipStream_t st);

// ao_amd/csrc/gva_plan.hip -- gva_plan(): the kernel form of every attention stage, decided in one place (gva_plan.h).
// Host code only.
#include "common.h"
#include "gva_plan.h"

GvaPlan gva_plan(int n, int k, int c, int g, bool attn_drop, bool has_inverse) {
    // the five path switches (common.h lists them); every one is read on every call
    const bool fwd_staged = ptv2_env_set("AO_AMD_FWD_STAGED");     // the three staged forward launches
    const bool bwd_staged = ptv2_env_set("AO_AMD_BWD_STAGED");     // the staged launches in every stage of the attention
    const bool bwd_point = ptv2_env_set("AO_AMD_BWD_POINT");       // peb_bwd + point kernel instead of the backward tile kernel
    const bool tile_keep_A = ptv2_env_set("AO_AMD_TILE_KEEP_A");   // the tile forward writes A, the strided weight gradient reads it
    const bool logits_bwd_staged = ptv2_env_is("AO_AMD_LOGITS_BWD", 's');  // "staged": the three-kernel logits backward

    GvaPlan P;
    P.g_slot = g == 6 ? 0 : g == 12 ? 1 : g == 24 ? 2 : g == 48 ? 3 : g == 64 ? 4 : -1;

    // ---- forward ----
    // (frozen: the logits forward is gated by AO_AMD_BWD_STAGED, not by AO_AMD_FWD_STAGED)
    P.logits_fwd = gva_logits_fwd_mfma_supported(k, c, g) && !bwd_staged ? GvaPlan::LF_MFMA
                   : k <= 16 && c % 4 == 0 && (g == 48 || g == 64) && !bwd_staged ? GvaPlan::LF_POINT  // pays for wide G only
                                                                                  : GvaPlan::LF_ROWS;
    // one launch at the full-resolution level (gva_fwd_point.hip), one per 16-point tile at the deep levels (gva_fwd_tile.hip)
    const bool fwd_tile = gva_fwd_tile_supported(k, c, g) && !fwd_staged;
    P.fwd = gva_fwd_point_supported(k, c, g) && n <= gva_fwd_point_max_n() && !attn_drop && !fwd_staged ? GvaPlan::F_POINT
            : fwd_tile                                                                                ? GvaPlan::F_TILE
                                                                                                      : GvaPlan::F_STAGED;
    // (frozen: the softmax of the staged forward follows AO_AMD_BWD_STAGED as well; g = 6 stays on the rows kernel)
    P.softmax = k <= 16 && (g == 12 || g == 24 || g == 48 || g == 64) && !bwd_staged ? GvaPlan::SM_POINT : GvaPlan::SM_ROWS;
    // (frozen: keeps_A ignores n and dropout although fwd depends on them -- the saved region is sized without knowing either;
    //  F_POINT and F_STAGED both write A, and only shapes without a point kernel reach F_TILE, so the two still agree)
    P.keeps_A = !fwd_tile || tile_keep_A;
    P.wp2_recompute = !P.keeps_A;  // no A: the weight gradient forms it again (gva_wgrad_tile.hip has the shapes of gva_fwd_tile.hip)

    // ---- backward ----
    P.bwd_tile_shape = gva_bwd_tile_supported(k, c, g) != 0;
    const bool point = gva_bwd_point_supported(k, c, g) && !bwd_staged;
    // handed g_A / g_sw: the fused point kernel gathers grad v through the inverse table, the staged kernels need none
    P.bwd_agg_given_gA = has_inverse && point ? GvaPlan::B_POINT : GvaPlan::B_STAGED;
    P.bwd_agg = P.bwd_tile_shape && !bwd_staged && !bwd_point    ? GvaPlan::B_TILE
                : gva_bwd_point_local(k, c, g) && !bwd_staged    ? GvaPlan::B_POINT_LOCAL
                                                                 : P.bwd_agg_given_gA;
    // (frozen, ADVICE finding 4: fused_peb does not look at has_inverse; the launchers return PTV2_ERR_ARG for fused_peb
    //  without the inverse table instead of falling back to a form that needs none)
    P.fused_peb = P.bwd_agg == GvaPlan::B_TILE || P.bwd_agg == GvaPlan::B_POINT_LOCAL;
    // (frozen: B_STAGED with attention dropout returns PTV2_ERR_ARG -- only the fused kernels apply the mask; every shape
    //  with a tile kernel has a point kernel too, so this is the whole condition)
    P.bwd_takes_dropout = point;
    // (frozen: gva_attention_backward_hip_launcher rejects every shape without bwd_tile_shape, also where B_POINT_LOCAL would run)
    P.logits_bwd = has_inverse && gva_logits_bwd_fused_supported(k, c, g) && !logits_bwd_staged && !bwd_staged ? GvaPlan::LB_FUSED
                   : g >= 48 && point ? GvaPlan::LB_ROWS_POINT_PARAMS  // pays for wide G only
                                      : GvaPlan::LB_ROWS_PARAMS;
    return P;
}

extern "C" int ptv2_gva_plan_describe(int n, int k, int c, int g, int attn_drop, int has_inverse, int *out, int out_len) {
    if (n < 0 || k < 1 || c < 1 || g < 1 || !out || out_len < GVA_PLAN_DESCRIBE_FIELDS) return PTV2_ERR_ARG;
    const GvaPlan P = gva_plan(n, k, c, g, attn_drop != 0, has_inverse != 0);
    const int v[GVA_PLAN_DESCRIBE_FIELDS] = {P.logits_fwd, P.fwd, P.softmax, P.bwd_agg, P.bwd_agg_given_gA, P.logits_bwd,
                                            P.keeps_A, P.fused_peb, P.wp2_recompute, P.bwd_takes_dropout, P.bwd_tile_shape,
                                            P.g_slot};
    for (int i = 0; i < GVA_PLAN_DESCRIBE_FIELDS; ++i) out[i] = v[i];
    return PTV2_OK;
}

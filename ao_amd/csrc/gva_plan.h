// ao_amd/csrc/gva_plan.h -- which kernel form every stage of one grouped-vector-attention call runs.
//
// gva_plan() (gva_plan.hip) is the one place that combines the shapes the kernels are instantiated for (the *_supported
// functions of their units) with the A/B switches of the environment.  A launcher entry computes the plan once at its top
// and hands it down; the sizing entry points (gva_block_workspace_bytes, ptv2_block_saved_bytes) consult the same function,
// so what is carved and what is run cannot disagree.
#pragma once

struct GvaPlan {
    enum LogitsFwd { LF_MFMA, LF_POINT, LF_ROWS };
    enum Fwd { F_POINT, F_TILE, F_STAGED };                       // softmax + aggregation + grouped projection
    enum Softmax { SM_POINT, SM_ROWS };                           // the softmax inside F_STAGED
    enum BwdAgg { B_TILE, B_POINT_LOCAL, B_POINT, B_STAGED };     // B_POINT: behind a peb_bwd launch (reads g_A / g_sw)
    enum LogitsBwd { LB_FUSED, LB_ROWS_POINT_PARAMS, LB_ROWS_PARAMS };
    LogitsFwd logits_fwd;
    Fwd fwd;
    Softmax softmax;
    BwdAgg bwd_agg;          // the Block's softmax / aggregation backward
    BwdAgg bwd_agg_given_gA; // ... of a caller that hands g_A / g_sw in (gva_aggregate_backward_hip_launcher): B_POINT | B_STAGED
    LogitsBwd logits_bwd;
    bool keeps_A;            // the forward writes A (n,g,c); block.hip sizes the saved region with it
    bool fused_peb;          // bwd_agg forms g_A / g_sw on chip: neither is carved, and the backward needs the inverse table
    bool wp2_recompute;      // grad Wp2 through gva_wgrad_tile (A formed again) instead of the strided form that reads A
    bool bwd_takes_dropout;  // a form of the backward that applies attention dropout exists (python: gva.dropout_supported)
    bool bwd_tile_shape;     // gva_bwd_tile.hip is instantiated for (k, c, g), whatever the switches say
    int g_slot;              // 0..4 for g in {6, 12, 24, 48, 64}, -1 otherwise: offset of the per-G kernel-timer ids
};

// attn_drop: attention dropout is active in this call; has_inverse: the caller hands the inverse neighbour table in.
// Reads the switches on every call (the parity tests flip them in-process).
GvaPlan gva_plan(int n, int k, int c, int g, bool attn_drop, bool has_inverse);

// ints that ptv2_gva_plan_describe() writes, in this order (include/ptv2_hip.h documents the same list)
enum { GVA_PLAN_DESCRIBE_FIELDS = 12 };

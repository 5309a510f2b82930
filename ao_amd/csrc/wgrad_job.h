// ao_amd/csrc/wgrad_job.h -- one weight-gradient call as its kernels and its finalize read it (wgrad.hip plans it once per call;
// launched at once it is the kernel's argument, by value; filed inside a model backward it is an entry of its kernel form's job
// table, run by one launch per form at the backward's end), shared with gva_wgrad_tile.hip.  What only the host needs (form,
// algorithmic bytes) stays out of it: eight of these are one 4 KB argument block of the table writer.
#pragma once

namespace dense {

struct WgradJob {
    int n, cout, cin, tiles_i, tiles, batch, chunk, chunks;
    int wg0;          // first workgroup of the job in the batched launch
    int has_pb, count;  // bias sums behind the weight records; > 0: the multi form (operand pairs per product)
    int rec, fin0;    // floats per chunk record; first element of the job in the batched finalize
    int wgs, gw;      // workgroups of the job; (grouped form) groups per workgroup
    int fin_lanes;    // record groups per output element in the batched finalize (1, or 4: the wavefronts of a workgroup)
    long long ldy, sy, ldx, sx, lds_s;
    const float *gY, *X, *rowscale;
    float *part;
    const float *mgY[6], *mX[6], *mxsc[6], *mxsh[6];
    float *dW, *db, *mdW[6], *mdb[6];  // finalize: strided form -> dW (batch * cout * cin) then db; multi form -> per product
    // recompute form (gva_wgrad_tile.hip: the grouped projection's weight gradient with A = w^T P formed again from the saved
    // softmax weights X = w (n,16,g), gY = g_out, rowscale = sw): aux = coord, idx (int), a, b; tiles = group blocks, tiles_i =
    // channel ranges, chunks = point splits
    const void *aux[4];
};

}  // namespace dense

/* gten_hip_oplanes.h: the A/B control of the single-sequence o projection -- one plane or four K-quarter planes, the same bytes --
 * beside the controls of include/gten_hip_ab.h (whose list of names a test pins, so this switch has a header of its own). */
#pragma once

#include "gten_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The o projection of single-sequence decoders created AFTERWARDS (a decoder keeps the choice it was created with: its graphs are
 * captured once), csrc/gten_decode_oplanes.h and DESIGN.md 3.2:
 *   1 (the default)  k_dec_o_planes -- one workgroup per (32 rows, K quarter) joins and stages only its quarter's eight heads and
 *                    stores its rows' quarter sums into one of four planes; the gate|up launch adds the planes in the order of the
 *                    one-plane kernel's own reduction tree, (p0 + p1) + (p2 + p3);
 *   0                k_dec_gemv8<.., PRO_ATTW, ..> -- every workgroup joins and stages the whole vector (the A/B control the
 *                    tests hold the planes to).
 * Both leave the same bytes everywhere behind the o launch (tests/test_decode_o_planes_gpu.py).  Any other value is an error.  The
 * planes apply to the fast forms with one-pass attention, Q8 activations (q4 or q8 weights) and n_embd 2048; f16, other widths,
 * decoders of 2+ sequences, the exact forms and the persistent step keep the one-plane launch whatever the setting. */
int gten_hip_set_decode_o_planes(int v);
/* the setting a decoder created now would read (a test puts it back with gten_hip_set_decode_o_planes) */
int gten_hip_decode_o_planes(void);
/* what a decoder chose: *planes = 1 (k_dec_o_planes) or 0 */
int gten_hip_decoder_o_planes(gten_hip_decoder* dec, int* planes);

#ifdef __cplusplus
}
#endif

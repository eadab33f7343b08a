/*
 * gten_hip_nucleus.h -- top-p (nucleus) and min-p truncation of the draw, on the device, as exact integer cuts; exported by
 * libgten_hip.so beside include/gten_hip_sample.h, include/gten_hip_bias.h and include/gten_hip_logprobs.h (same conventions:
 * device pointers unless the name ends in _host, 0 on success, otherwise a code with gten_hip_last_error()).
 *
 * The contract (it amends §3.7 / §3.10 only where a cut is set).  A sequence's request gains (top_p, min_p)
 * beside (top_k, temp, seed, stream): 0 < top_p <= 1, 0 <= min_p <= 1, both finite; anything else is refused with a code.
 * top_p == 1 && min_p == 0 is "no cut": such a sequence runs exactly the draw of §3.7 and produces the same ids bit for bit.
 * A greedy sequence (top_k == 0) ignores the cut.  Nucleus sampling over the whole vocabulary is top_k >= n_vocab.
 *
 * For the row y (x, or x + b under a bias table that holds), mx = max y:
 *   1. candidates  C = the candidate set of §3.7, ordered key descending, index ascending (the order of the log-prob records);
 *   2. scores      a_j = (y_j - mx) / temp in f32 -- the expression the draw scores with;
 *   3. masses      w_j = expf(a_j); q_j = (uint64) floorf(w_j * 2^36) (the multiply is exact, the largest q is 2^36, -inf gives
 *                  0); Z = sum over C of q_j in u64 (n_vocab <= 65535: Z < 2^52).  Integer addition is associative: Z and every
 *                  partial sum are independent of the reduction order;
 *   4. nucleus     P = (uint64) floor((double)Z * (double)top_p), one IEEE f64 multiply; n_nucleus = the length of the
 *                  shortest non-empty prefix of C whose mass is >= P (top_p == 1: n_nucleus = |C|).  Ties at the cut key have
 *                  equal q, so the number of them taken is an integer division; they go to the lower index;
 *   5. min-p       t = (float)log((double)min_p), computed once on the host when the request is set (-inf for min_p == 0);
 *                  n_minp = #{j in C : a_j >= t} -- a prefix of C, a is monotone in the key; the comparison is exact;
 *   6. draw        F = the first n_keep = min(n_nucleus, n_minp) of C (n_keep >= 1: the maximum always survives);
 *                  id = argmax over F of a_j + g_j with §3.7's noise and tie rule.  If the uncut id lies in F, the cut id is it.
 * Log-prob records (§3.11) stay computed from the raw row.  A slot that repeats its step rewrites the same id.  NaN or +inf
 * in a row is outside the contract.  Nothing here depends on the slot, the lane, the schedule or a float summation order.
 */
#ifndef GTEN_HIP_NUCLEUS_H
#define GTEN_HIP_NUCLEUS_H

#include <stdint.h>

#include "gten_hip_sample.h"

#define GTEN_HIP_NUCLEUS_MASS_BITS 36
#define GTEN_HIP_NUCLEUS_INFO_BYTES 24

#ifdef __cplusplus
extern "C" {
#endif

/* What gten_hip_sample_rows_cut reports per row (all zero for a greedy row). */
typedef struct gten_hip_cut_info {
    uint64_t Z;
    int32_t n_cand, n_nucleus, n_minp, n_keep;
} gten_hip_cut_info;

/* Sequence `seq` draws under the cut (top_p, min_p) from now on; (1, 0) clears it.  It is part of the sequence's request
 * beside gten_hip_decoder_set_sampling's, gten_hip_decoder_set_seq_bias's and gten_hip_decoder_set_logprobs's, which leave it
 * alone.  The decoder's first cut allocates the per-sequence array and drops its captured graphs once; while no sequence has
 * ever set one, the step launches exactly the kernels it did.  Refused: top_p outside (0, 1], min_p outside [0, 1], NaN, a
 * cut on a decoder created with the persistent step. */
int gten_hip_decoder_set_cut(gten_hip_decoder* dec, int seq, float top_p, float min_p);

/* top_p_host / min_p_host / t_host (each [n_seq] or NULL): every sequence's cut ((1, 0, -inf): none); *on (may be NULL):
 * whether a sequence of the decoder has ever set a cut. */
int gten_hip_decoder_cut_info(gten_hip_decoder* dec, float* top_p_host, float* min_p_host, float* t_host, int* on);

/* gten_hip_sample_rows_biased (bias may be NULL: y = x) with row r cut by (top_p_host[r], min_p_host[r]); info_out (device,
 * [n_rows] gten_hip_cut_info, may be NULL).  The same row routine as the decoder's.  A row with no cut draws by the routine of
 * gten_hip_sample_rows unless info_out is given (then by the cut routine with F = C: the same id).  Synchronous. */
int gten_hip_sample_rows_cut(const float* logits, int n_rows, int n_vocab, long long row_stride, const float* bias, long long bias_stride,
                             const int32_t* top_k_host, const float* temp_host, uint64_t seed, const uint32_t* stream_host,
                             const int32_t* position_host, const float* top_p_host, const float* min_p_host, int32_t* out,
                             gten_hip_cut_info* info_out);

#ifdef __cplusplus
}
#endif
#endif

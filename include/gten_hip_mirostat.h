/*
 * gten_hip_mirostat.h -- Mirostat v2 sampling on the device: integer surprise, mu per position; exported by libgten_hip.so beside
 * include/gten_hip_nucleus.h and include/gten_hip_fsm.h (same conventions: device pointers unless the name ends in _host, 0 on
 * success, otherwise a code with gten_hip_last_error()).
 *
 * The contract (it amends §3.7, §3.14 and §3.15 only where a sequence is bound).  Mirostat holds the surprise of the
 * generated text at a target tau: it keeps a running threshold mu, drops every candidate more surprising than mu, and after each id
 * moves mu by eta * (tau - observed surprise).  Surprise, tau, eta and mu are int32 in units of 2^-16 bit (Q16):
 *   tau_q = (int32) lrint((double)tau * 65536), eta_q likewise, formed once on the host when the request is set; 0 < tau <= 32,
 *   0 < eta <= 1, both finite, anything else is refused with a code; |mu| <= GTEN_HIP_MIRO_MU_MAX; the default start is 2 * tau_q.
 *
 * lg16(x) for a uint64 x >= 1 -- a definition, not an approximation:
 *   e = 63 - clz(x);  m = e >= 31 ? x >> (e - 31) : x << (31 - e)                  (2^31 <= m < 2^32)
 *   f = 0;  16 times: m = (m * m) >> 31 (u64 product); f <<= 1; if m >= 2^32: f |= 1, m >>= 1
 *   lg16 = (e << 16) | f
 * It is monotone non-decreasing in x, lg16(1) = 0, lg16(2^36) = 36 << 16.
 *
 * The step, for a bound sequence that samples (top_k >= 1), on the row y the draw sees (the penalty first, then the bias table or the
 * automaton's mask):
 *   1. C, mx, a_j = (y_j - mx) / temp in f32, q_j = (uint64) floorf(expf(a_j) * 2^36), Z = sum over C of q_j: include/gten_hip_nucleus.h's
 *      steps 1 to 3, unchanged;
 *   2. L = lg16(Z) - mu, mu = mu_row[n]; the kept set F = {the first of C} + {j in C : q_j >= 1 and lg16(q_j) >= L}.  q is monotone
 *      in the key and lg16 in q, so F is the first n_keep of C, n_keep >= 1;
 *   3. id = argmax over F of a_j + g_j with §3.7's noise and tie rule;
 *   4. Zk = sum over F of q_j; s = lg16(Zk) - lg16(q_id)  (q_id >= 1 always);
 *   5. mu' = clamp(mu - (int32)(((int64)eta_q * (int64)(s - tau_q)) >> 16), -MU_MAX, MU_MAX), the shift arithmetic; the thread that
 *      commits the id writes mu_row[n + 1] = mu'.
 * No float enters a decision except a_j and expf.  A greedy sequence ignores Mirostat (its mu row is not touched).  Log-prob records stay
 * on the raw row.  A slot that repeats its step reads the same mu_row[n] and rewrites the same mu_row[n + 1].  A sequence bound at pos
 * never looks behind it.  A cut other than (1, 0) and Mirostat on one sequence are refused by whichever setter would create the pair.
 * A decoder created with the persistent step refuses Mirostat.
 */
#ifndef GTEN_HIP_MIROSTAT_H
#define GTEN_HIP_MIROSTAT_H

#include <stdint.h>

#include "gten_hip_fsm.h"

#define GTEN_HIP_MIRO_MU_MAX (64 << 16)
#define GTEN_HIP_MIRO_MU_DEFAULT INT32_MIN      /* "start at 2 * tau_q" */
#define GTEN_HIP_MIRO_INFO_BYTES 48

/* what gten_hip_miro_q16_host answers */
#define GTEN_HIP_MIRO_OK 0
#define GTEN_HIP_MIRO_BAD_TAU 1                 /* tau outside (0, 32], or not finite */
#define GTEN_HIP_MIRO_BAD_ETA 2                 /* eta outside (0, 1], or not finite */

#ifdef __cplusplus
extern "C" {
#endif

/* What gten_hip_sample_rows_miro reports per row.  A greedy row and a row with tau 0: all zero but mu_next, which is the row's mu. */
typedef struct gten_hip_miro_info {
    uint64_t Z, Zk, q_id;
    int32_t n_cand, n_keep, s, mu_next, pad[2];
} gten_hip_miro_info;

/* The shared arithmetic (csrc/gten_miro_math.h), device-free: these three need no device and no gten_hip_init.
 * lg16(x) (0 for x == 0, which is outside the definition); the update of step 5; a request to Q16 (one of the codes above; on
 * GTEN_HIP_MIRO_OK *tau_q and *eta_q are written). */
int32_t gten_hip_miro_lg16_host(uint64_t x);
int32_t gten_hip_miro_update_host(int32_t mu, int32_t s, int32_t tau_q, int32_t eta_q);
int gten_hip_miro_q16_host(float tau, float eta, int32_t* tau_q, int32_t* eta_q);

/* "The id that will sit at position pos of sequence seq, and every later one, is drawn under Mirostat (tau, eta), starting from
 * mu_q16" (GTEN_HIP_MIRO_MU_DEFAULT: 2 * tau_q); it writes mu_row[pos].  tau == 0 unbinds the sequence (eta, mu_q16 and pos are then
 * not looked at).  pos in [1, max_ctx].  The decoder's first binding allocates the per-sequence arrays and drops its captured graphs
 * once; while no sequence has ever been bound, the step launches exactly the kernels it did.  Refused: tau or eta outside their ranges,
 * |mu_q16| > GTEN_HIP_MIRO_MU_MAX, a sequence whose cut is on (and gten_hip_decoder_set_cut refuses a cut on a sequence bound here), a
 * decoder created with the persistent step. */
int gten_hip_decoder_set_seq_mirostat(gten_hip_decoder* dec, int seq, float tau, float eta, int32_t mu_q16, int pos);

/* tau_q_host / eta_q_host / pos_host ([n_seq] or NULL): every sequence's binding (0, 0, 0: unbound); *on: whether a sequence has ever
 * been bound; row_host (or NULL): a copy of sequence row_seq's mu row, entries [row_from, row_from + row_count) of its max_ctx + 2
 * (zeros while nobody has ever been bound). */
int gten_hip_decoder_mirostat_info(gten_hip_decoder* dec, int32_t* tau_q_host, int32_t* eta_q_host, int32_t* pos_host, int* on, int row_seq,
                                   int row_from, int row_count, int32_t* row_host);

/* gten_hip_decoder_slot_states for the mu rows: entries [n_from, n_from + count) of sequence seq's row, n_from + count <= max_ctx + 2.
 * out_host[i] is the mu the id at position n_from + i was (or will be) drawn under. */
int gten_hip_decoder_slot_mus(gten_hip_decoder* dec, int seq, int n_from, int count, int32_t* out_host);

/* gten_hip_sample_rows_fsm without the cut arrays, with an optional bias row as in gten_hip_sample_rows_cut (bias NULL: none), row r
 * drawn under Mirostat (tau_host[r], eta_host[r]) with the threshold mu_host[r] (Q16).  tau_host[r] == 0: the row draws by the routine
 * of gten_hip_sample_rows_fsm / gten_hip_sample_rows_cut at the cut (1, 0).  The pool is optional: (next, flags, state_host) all NULL
 * and n_states 0 is "no row is in a state".  A bias beside a row in a state (state_host[r] >= 0) is refused.  hist_offset_host NULL: no
 * penalties.  next_state_out and info_out (device, [n_rows], may be NULL); info_out[r].mu_next is what a decoder would write to
 * mu_row[n + 1].  The same row routine as the decoder's; it draws a prompt's first id.  Synchronous. */
int gten_hip_sample_rows_miro(const float* logits, int n_rows, int n_vocab, long long row_stride, const float* bias, long long bias_stride,
                              const uint16_t* next, const uint8_t* flags, int n_states, const int32_t* state_host, const int32_t* top_k_host,
                              const float* temp_host, uint64_t seed, const uint32_t* stream_host, const int32_t* position_host,
                              const int32_t* hist_host, const int32_t* hist_offset_host, const float* r_host, const float* freq_host,
                              const float* pres_host, const int32_t* mu_host, const float* tau_host, const float* eta_host, int32_t* out,
                              int32_t* next_state_out, gten_hip_miro_info* info_out);

#ifdef __cplusplus
}
#endif
#endif

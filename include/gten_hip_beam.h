/*
 * gten_hip_beam.h -- beam search on the device: the round that decides which (parent beam, id) pairs survive, and the in-place
 * gather that moves the K / V rows of a group's beams behind their parents; exported by libgten_hip.so beside
 * include/gten_hip_logprobs.h (same conventions: device pointers unless the name ends in _host, 0 on success, otherwise a code
 * with gten_hip_last_error()).  DESIGN.md §3.19.
 *
 * A GROUP is B = n_beams in [1, GTEN_HIP_BEAM_MAX] hypotheses of one prompt.  Beam b of a group owns list row row0 + b: the
 * ordered top 2B (id, x - lse) of its logits row -- exactly what gten_hip_row_top_logprobs(row, n_top = 2B) writes, which is why
 * 2 * GTEN_HIP_BEAM_MAX <= GTEN_HIP_LOGPROBS_TOP.
 *
 * ONE ROUND of a group, all in f32, every operation rounded once (no sum is reordered: the result does not depend on the launch):
 *   - a group that is done, or whose t has reached max_new, is left alone (done: not one byte of it changes);
 *   - otherwise t += 1; the sources are beams [0, n_src), n_src = 1 when t == 1 (every beam holds the same prompt), else B;
 *   - candidates (score = cum[b] + top_lp[b][r], b, r, id = top_id[b][r]) for every source b and r < 2B;
 *   - order: score descending (compared as floats, -0 == +0), then b ascending, then r ascending; the first 2B are walked by rank k:
 *       id == eos and k <  B: a hypothesis finishes with the record (final = score * w[t], cum = score, t, beam = b);
 *       id == eos and k >= B: dropped;
 *       id != eos: the next beam n_next++ with (parent = b, id, cum = score);
 *     the walk ends once n_next == B (a source lists eos at most once, so at least B of the 2B are not eos);
 *   - finished records fill slots 0 .. B - 1 (n_fin counts the filled slots); with all B full the new record replaces the slot with
 *     the smallest final (ties: the highest slot index), and only if its final is strictly greater;
 *   - done = n_fin >= B after the round (early stopping, the only rule);
 *   - written: the trellis rows parent[t][0..B) and id[t][0..B), the new cum, stepped = 1, and next_id[row0 + b] = id[t][b].
 */
#ifndef GTEN_HIP_BEAM_H
#define GTEN_HIP_BEAM_H

#include <stddef.h>
#include <stdint.h>

#include "gten_hip.h"
#include "gten_hip_logprobs.h"

#define GTEN_HIP_BEAM_MAX 8

#ifdef __cplusplus
extern "C" {
#endif

/* what a round needs to know of a group (device array [n_groups] for gten_hip_beam_round; host array for the decoder form, where
 * row0 is the group's first sequence and prompt_len its prompt's length) */
typedef struct {
    int32_t row0;               /* first list row / first sequence; the group's rows are row0 .. row0 + n_beams - 1 */
    int32_t n_beams;
    int32_t prompt_len;         /* decoder form only */
    int32_t max_new;            /* rounds the group may take: the trellis holds rows [0, max_new] */
    int32_t eos;                /* -1: none */
} gten_hip_beam_group;

/* a group's state between rounds: 176 bytes, all zero before round 1 */
typedef struct {
    float cum[GTEN_HIP_BEAM_MAX];
    float fin_final[GTEN_HIP_BEAM_MAX];
    float fin_cum[GTEN_HIP_BEAM_MAX];
    int32_t fin_t[GTEN_HIP_BEAM_MAX];
    int32_t fin_beam[GTEN_HIP_BEAM_MAX];
    int32_t n_fin, done, t;
    int32_t stepped;            /* the last round call advanced this group (what gten_hip_permute_sets moves rows for) */
} gten_hip_beam_state;

/* One round for n_groups groups (at most 65535).  top_id / top_lp: list row i at + i * row_stride elements (row_stride >= 2 * the
 * largest n_beams); w[n_w]: the length weights, w[t] read for t <= max_new (refused on the host side where it can be seen: the
 * kernel leaves a group alone whose next t is not below n_w); parent / ids: the trellis, [n_groups][trellis_rows][GTEN_HIP_BEAM_MAX]
 * (a group with t + 1 >= trellis_rows is left alone); next_id [list rows].  Asynchronous on the current stream.  The groups' fields
 * are read on the device: n_beams outside [1, 8], or a row_stride below 2 * n_beams (overlapping lists), makes the kernel leave the
 * group alone. */
int gten_hip_beam_round(const gten_hip_beam_group* groups, int n_groups, gten_hip_beam_state* state, const int32_t* top_id, const float* top_lp,
                        long long row_stride, const float* w, int n_w, int32_t* parent, int32_t* ids, int trellis_rows, int32_t* next_id);

/* The in-place gather across the B sets of a group.  ranges_host[n_ranges] (at most 65535): range i belongs to group `group` and
 * names B bases; afterwards base[b][offset .. offset + bytes) holds what base[parent[b]][offset ..) held before, for every b at
 * once, any permutation or duplication included.  bytes and offset are multiples of 4, the bases 4-byte aligned.
 *   state == NULL: parent is [n_groups][GTEN_HIP_BEAM_MAX], group g's row at parent + g * 8 (trellis_rows ignored);
 *   state != NULL: parent is the trellis of gten_hip_beam_round; group g takes row state[g].t, and is skipped when it is done or
 *                  its last round did not advance it.
 * A thread owns one piece -- the same offset in all B sets --, loads it from every set it needs and then stores: no other thread
 * touches that offset, so there is no barrier and no second buffer.  16-byte pieces where offset, bytes and every base allow it,
 * else 4-byte pieces.  A group whose parent is the identity is skipped, a set with parent[b] == b is not stored, an entry outside
 * [0, B) counts as b.  Asynchronous; every range is announced to the head-major shadows' watch registry. */
typedef struct {
    void* base[GTEN_HIP_BEAM_MAX];
    int32_t group;
    int32_t pad;
} gten_hip_permute_range;
int gten_hip_permute_sets(const gten_hip_permute_range* ranges_host, int n_ranges, size_t offset, size_t bytes, const gten_hip_beam_group* groups,
                          int n_groups, const gten_hip_beam_state* state, const int32_t* parent, int trellis_rows);

/* ---- the decoder form: G groups on the sequences of one multi-sequence decoder.
 * begin: group g's sequences row0 .. row0 + n_beams - 1 each hold the prompt's ids [0, prompt_len) (gten_hip_decoder_set_tokens_seq)
 *   and its K / V rows [0, prompt_len - 1).  w_host[n_w] with n_w > every max_new.  Allocates the state, the trellis and the range
 *   tables, remembers the sequences' log-prob requests and replaces them by n_top = 2 * n_beams (the lists are the step's own
 *   records; the graphs are dropped only if this is the decoder's first log-prob request), starts the groups'
 *   slots at n = prompt_len and parks every other sequence.  Refused: n_beams outside [1, 8]; groups that overlap or pass n_seq;
 *   prompt_len < 1, max_new < 1, prompt_len + max_new > max_ctx; 2 * n_beams > n_vocab; a persistent-step decoder; a sequence that
 *   samples, is bound to a bias table or an automaton, or is penalised; a search already begun.
 * round: asynchronous: one shared step of the decoder, then the round over the step's records (the chosen ids go into the
 *   sequences' token rows, where the next step embeds them), then the gather over rows [prompt_len - 1, prompt_len - 1 + rounds) of
 *   every layer's K and V -- from round 2 on: in round 1 every beam wrote the same bytes into row prompt_len - 1, nothing moves.
 *   At most min(max_new) rounds.
 * live: waits for the stream; *n_live = groups not done (4 bytes come back).
 * read: waits; group g's state and trellis rows [1, t]: parent_host / ids_host [t][GTEN_HIP_BEAM_MAX] (room for max_new rows).
 * end: restores the sequences' requests and parks the groups' slots; the decoder steps, generates and serves as before. */
int gten_hip_decoder_beam_begin(gten_hip_decoder* dec, const gten_hip_beam_group* groups_host, int n_groups, const float* w_host, int n_w);
int gten_hip_decoder_beam_round(gten_hip_decoder* dec);
int gten_hip_decoder_beam_live(gten_hip_decoder* dec, int* n_live);
int gten_hip_decoder_beam_read(gten_hip_decoder* dec, int g, gten_hip_beam_state* state_host, int32_t* parent_host, int32_t* ids_host);
int gten_hip_decoder_beam_end(gten_hip_decoder* dec);
/* rounds run since begin, the bytes one gather launch covered last (all sets of all groups) and its launches so far */
int gten_hip_decoder_beam_info(gten_hip_decoder* dec, int* rounds, unsigned long long* permute_bytes, unsigned long long* permute_launches);

#ifdef __cplusplus
}
#endif
#endif

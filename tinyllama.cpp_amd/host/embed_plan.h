// embed_plan.h -- which texts of an embedding call share a prompt pass.  Device-free: integers in, integers out;
// exported as gten_host_embed_plan (include/gten_host_embed.h), restated by tests/embed_ref.py and exercised under sanitizers by
// tests/host_embed_plan.cpp.
//
// It is the rule TinyLlama::score_many follows (host/tinyllama_model.h), stated once.  Texts are taken in order.  A text of
// 16 .. 2048 ids is GROUPED where the configuration has a segmented prompt path (seg_ok, gten_hip_row_segments_ok): it joins the
// open group unless that group already holds 32 texts or would pass 4096 rows, in which case it opens a new one.  Every other
// text goes ALONE, a group of one that does not close the open group.  Groups are numbered in the order of their first texts.
#pragma once

namespace gten {

constexpr int kEmbedGroupTexts = 32;     // texts of one group (TinyLlama::kScoreTexts)
constexpr int kEmbedGroupRows = 4096;    // rows of one group (TinyLlama::kScoreRows)
constexpr int kEmbedGroupMin = 16;       // the shortest text that is grouped
constexpr int kEmbedGroupMax = 2048;     // the longest

inline bool embed_grouped(int len, bool seg_ok) { return seg_ok && len >= kEmbedGroupMin && len <= kEmbedGroupMax; }

// group_of[k] = the group of text k, alone[g] = 1 where group g is a text that goes alone (either may be null; alone has room for
// n_texts entries).  Returns the number of groups, or -1 for no texts or a text without ids.
inline int embed_plan(const int* lengths, int n_texts, bool seg_ok, int* group_of, int* alone)
{
    if (!lengths || n_texts < 1) return -1;
    for (int k = 0; k < n_texts; k++)
        if (lengths[k] < 1) return -1;
    int n_groups = 0, open = -1, open_texts = 0, open_rows = 0;
    for (int k = 0; k < n_texts; k++) {
        const int len = lengths[k];
        if (!embed_grouped(len, seg_ok)) {
            if (alone) alone[n_groups] = 1;
            if (group_of) group_of[k] = n_groups;
            n_groups++;
            continue;
        }
        if (open < 0 || open_texts == kEmbedGroupTexts || open_rows + len > kEmbedGroupRows) {
            open = n_groups++;
            open_texts = open_rows = 0;
            if (alone) alone[open] = 0;
        }
        if (group_of) group_of[k] = open;
        open_texts++;
        open_rows += len;
    }
    return n_groups;
}

} // namespace gten

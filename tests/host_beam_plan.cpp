// host_beam_plan.cpp -- hand-written cases for host/beam_plan.h (the length weights, the walk back through a trellis, the final
// ranking), built with -fsanitize=address,undefined by tests/test_beam_cpu.py.  Includes that header alone: no device, no model.
#include "../tinyllama.cpp_amd/host/beam_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace gten;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "host_beam_plan: line %d: %s\n", __LINE__, #cond); \
            std::exit(1);                                                           \
        }                                                                           \
    } while (0)

static bool same(const std::vector<int32_t>& a, std::initializer_list<int32_t> b) { return a == std::vector<int32_t>(b); }

static void weights()
{
    const std::vector<float> one = beam_weights(4, 1.f);
    CHECK(one.size() == 5 && one[0] == 0.f && one[1] == 1.f && one[2] == 0.5f && one[3] == (float)(1.0 / 3.0) && one[4] == 0.25f);
    const std::vector<float> none = beam_weights(3, 0.f);
    CHECK(none[0] == 0.f && none[1] == 1.f && none[2] == 1.f && none[3] == 1.f);
    const std::vector<float> two = beam_weights(3, 2.f);
    CHECK(two[2] == 0.25f && two[3] == (float)(1.0 / 9.0));
    const std::vector<float> half = beam_weights(4, 0.5f);
    CHECK(half[4] == 0.5f && half[2] == (float)(1.0 / std::sqrt(2.0)));
    CHECK(beam_weights(0, 1.f).size() == 1 && beam_weights(-3, 1.f).size() == 1);
}

// three rounds, B = 3: round 2 duplicates beam 0 and drops beam 2, round 3 crosses
static const int32_t kParent[3 * kBeamMax] = {0, 0, 0, 0, 0, 0, 0, 0, /**/ 0, 0, 1, 0, 0, 0, 0, 0, /**/ 2, 0, 1, 0, 0, 0, 0, 0};
static const int32_t kIds[3 * kBeamMax] = {10, 11, 12, 0, 0, 0, 0, 0, /**/ 20, 21, 22, 0, 0, 0, 0, 0, /**/ 30, 31, 32, 0, 0, 0, 0, 0};

static void backtrack()
{
    const BeamTrellis tr{kParent, kIds, 3};
    CHECK(beam_backtrack(tr, 0, 0).empty());
    CHECK(same(beam_backtrack(tr, 1, 2), {12}));
    CHECK(same(beam_backtrack(tr, 2, 0), {10, 20}) && same(beam_backtrack(tr, 2, 1), {10, 21}) && same(beam_backtrack(tr, 2, 2), {11, 22}));
    CHECK(same(beam_backtrack(tr, 3, 0), {11, 22, 30}) && same(beam_backtrack(tr, 3, 1), {10, 20, 31}) && same(beam_backtrack(tr, 3, 2), {10, 21, 32}));
    CHECK(beam_backtrack(tr, 4, 0).empty() && beam_backtrack(tr, 2, 8).empty() && beam_backtrack(tr, 2, -1).empty() && beam_backtrack(tr, -1, 0).empty());
    int32_t bad[3 * kBeamMax];
    std::memcpy(bad, kParent, sizeof(bad));
    bad[2 * kBeamMax] = 9;                                    // a parent outside the trellis
    CHECK(beam_backtrack(BeamTrellis{bad, kIds, 3}, 3, 0).empty());
}

static void finalize()
{
    const BeamTrellis tr{kParent, kIds, 3};
    const std::vector<float> w = beam_weights(3, 1.f);
    // none finished: the live beams by cum * w[3]; beams 0 and 2 tie, the lower beam first
    BeamState st{};
    st.t = 3;
    st.cum[0] = -3.f; st.cum[1] = -1.5f; st.cum[2] = -3.f;
    std::vector<BeamHypothesis> h = beam_finalize(st, tr, 3, w.data());
    CHECK(h.size() == 3 && same(h[0].ids, {10, 20, 31}) && h[0].final_score == -0.5f && h[0].cum == -1.5f && h[0].ended_by == kBeamEndedLength);
    CHECK(same(h[1].ids, {11, 22, 30}) && same(h[2].ids, {10, 21, 32}) && h[1].final_score == -1.f && h[2].final_score == -1.f);
    // some finished: one at round 2 from beam 1 (= beam 1 after round 1), one at round 3 from beam 2 (= beam 2 after round 2); the
    // first ties with live beam 1: finished before live
    st.n_fin = 2;
    st.fin_final[0] = -0.5f; st.fin_cum[0] = -1.f; st.fin_t[0] = 2; st.fin_beam[0] = 1;
    st.fin_final[1] = -2.f; st.fin_cum[1] = -6.f; st.fin_t[1] = 3; st.fin_beam[1] = 2;
    h = beam_finalize(st, tr, 3, w.data());
    CHECK(h.size() == 3 && same(h[0].ids, {11}) && h[0].ended_by == kBeamEndedEos && h[0].cum == -1.f && h[0].final_score == -0.5f);
    CHECK(same(h[1].ids, {10, 20, 31}) && h[1].ended_by == kBeamEndedLength && same(h[2].ids, {11, 22, 30}) && h[2].ended_by == kBeamEndedLength);
    // B finished (done): the live beams are out however good; slots 0 and 2 tie, the lower slot first; a hypothesis finished at
    // round 1 has no ids
    st.n_fin = 3;
    st.done = 1;
    st.fin_final[2] = -0.5f; st.fin_cum[2] = -0.5f; st.fin_t[2] = 1; st.fin_beam[2] = 0;
    st.cum[1] = 0.f;
    h = beam_finalize(st, tr, 3, w.data());
    CHECK(h.size() == 3 && same(h[0].ids, {11}) && h[1].ids.empty() && h[1].cum == -0.5f && same(h[2].ids, {11, 22}));
    CHECK(h[0].ended_by == kBeamEndedEos && h[1].ended_by == kBeamEndedEos && h[2].ended_by == kBeamEndedEos && h[2].final_score == -2.f);
    // one beam; before any round; -0 and +0 are one value (the lower beam first)
    BeamState one{};
    one.t = 3;
    one.cum[0] = -6.f;
    h = beam_finalize(one, tr, 1, w.data());
    CHECK(h.size() == 1 && same(h[0].ids, {11, 22, 30}) && h[0].final_score == -2.f);
    CHECK(beam_finalize(BeamState{}, BeamTrellis{nullptr, nullptr, 0}, 4, w.data()).empty());
    BeamState z{};
    z.t = 1;
    z.cum[0] = 0.f; z.cum[1] = -0.f;
    h = beam_finalize(z, tr, 2, w.data());
    CHECK(h.size() == 2 && same(h[0].ids, {10}) && same(h[1].ids, {11}));
}

int main()
{
    weights();
    backtrack();
    finalize();
    std::printf("host_beam_plan ok\n");
    return 0;
}

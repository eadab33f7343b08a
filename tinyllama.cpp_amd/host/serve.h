// serve.h -- continuous batching: the scheduler behind TinyLlamaBatch::serve_with (host/tinyllama_model.h, which includes this
// file at its end).  What it DECIDES is host/serve_plan.h, device-free and tested on the CPU; this file is what it
// DOES with the decoder.  Like tinyllama_model.h it names only entry points of include/gten_hip.h -- prefixes, group records and
// continued rows go through the detail:: hooks.
//
// Every prompt is generated greedily to `max_tokens` ids in all (prompt included) or until `eos` (not stored,
// tinyllama.cpp:425), as greedy_sample does for one sequence; max_new > 0 additionally bounds the new ids per prompt.
// One host thread keeps two things going that OVERLAP on the GPU:
//   * a slice of `slice` shared free-running steps of the live slots, queued on stream 0 (gten_hip_decoder_run);
//   * while it runs: the prompts of the next sequences, one after the other, each on a free slot's own caches on stream 1
//     (operator path: iteration 0 of the reference's loop incl. the host argmax of its logits).  A parked slot idles on
//     the decoder's dummy caches (gten_hip_decoder_slot_park), so nothing the shared steps do touches the caches being
//     filled.  Prompt processing is host-bound (~500 short launches) and the shared steps are GPU-bound: side by side
//     they hide each other.
// Between two prompts the slice is polled (gten_hip_stream_idle): once done its ids are read (eos / length -> the slot is
// parked and becomes free) and the next slice starts at once with the slots whose prompts became ready meanwhile.  Nobody
// runs past its last step: a slot that ends inside a slice repeats that step until the slice is over
// (gten_hip_decoder_slot_start_until; cutting the slice to the shortest remaining run instead left 128 slots with
// slices of one to three steps and prompt batches of two).  Per sequence the ids are those of
// generating it alone (bit for bit up to 8 slots; tests/test_serving_gpu.py).
// (lane_steps: shared steps x the lanes each of them ran -- a lane whose slots are all parked is left out of a run; lane_rows:
//  slots per lane; new ids / (lane_steps x lane_rows) is the share of COMPUTED slot-steps that produced an id)
// How the ids are picked is `pick`'s business (host/generate.h, ServePolicy): the first id of a prompt processed onto a cache
// set (first / many), the requests of the slot that takes it (apply), its log-prob records (collect), everything off again (clear).
// With Pick::kFsm a prompt may be bound to a token automaton (include/gten_hip_fsm.h): the id that enters a final state ends it as
// an eos does but is kept (ended_first / states / enters_final), and its binding is set again wherever it goes on (bind_state).
// (max_new[j] > 0 additionally bounds the new ids of prompt j)
// SAMPLE GROUPS (include/gten_host_samples.h): group_of[j] >= 0 names the group of queue item j; consecutive items
// of one group hold THE SAME PROMPT -- the caller's word, no prompt is compared.  prepare_batch takes whole groups while free
// sets and rows allow: the first member taken is computed, the others are copies of it (prefill_many_with's copy_of); a group
// that does not fit is cut, and what is left is a later group with a prompt pass of its own.  Ids and records are those of
// the same items without groups.  Sets written for a group of at least two readied members behind at least one full chunk carry
// a group mark; a slot started on such a set reads the prompt's full chunks from a group record of the decoder (GroupRecords).
// SESSION ITEMS (session[j] = s >= 0; the caller has checked that s is open and named once): prompts[j] is
// the session's ids + the turn's, and the item is that prompt in every respect but two -- its cache set is the session's own
// (never out of `pool`, never back into it) and only the rows the plan asks for are computed (prepare_batch's continued
// items).  When the item ends the session takes the out row as its ids.
#pragma once

#include "serve_plan.h"
#include "tinyllama_model.h"

namespace gten {

template <class Pick>
class ServeQueue {
    using clock = std::chrono::steady_clock;
    using ServeStats = TinyLlamaBatch::ServeStats;

    // one decode slot: prompt index (-1: free -- a slot is live iff it has a job), next step, last step, the cache set it decodes
    // on (-1: none), and (Pick::kLogprobs) the first position whose record the slot has not handed over
    struct Slot { int job = -1, cur = 0, last = 0, set = -1, lp_from = 0; };
    // a processed prompt waiting for a slot
    struct Ready { int j, set, cur, last; };
    // gten_hip_decoder_slots_apply's arguments: all joining slots in one call (their ids, step words and cache-table rows go up
    // behind each other, one wait), or all slots that are parked
    struct SlotsApply {
        std::vector<int> seq, first, last;
        std::vector<const int32_t*> tok;                                   // (joins only)
        void clear() { seq.clear(); first.clear(); last.clear(); tok.clear(); }
        void join(int q, int cur, int last_step, const int32_t* ids) { seq.push_back(q); first.push_back(cur); last.push_back(last_step); tok.push_back(ids); }
        void park(int q) { seq.push_back(q); first.push_back(0); last.push_back(0); }
        void send(gten_hip_decoder* dec)
        {
            if (!seq.empty()) GTEN_HIP_OK(gten_hip_decoder_slots_apply(dec, (int)seq.size(), seq.data(), first.data(), last.data(), tok.empty() ? nullptr : tok.data()));
        }
    };

    // Whatever way the queue is left (a failed check ends the process, but an allocation may throw), every slot goes back
    // to its own sequence's caches: a decoder left bound to spare or foreign sets would read and write the wrong rows in the
    // decode_step / generate that follows -- and dangle once share_weights() drops the spares.
    // (while the queue runs, cache sets are bound to slots by the scheduler and carry their "shares P rows" marks with them; the
    //  slots go back to their own sets afterwards, so no mark outlives the queue -- however it is left)
    struct ServeMarks {
        TinyLlamaBatch* b;
        explicit ServeMarks(TinyLlamaBatch* b_) : b{b_} { b->in_serve_ = true; }
        ~ServeMarks()
        {
            b->in_serve_ = false;
            // (a SESSION's set keeps its mark between queues: its rows stay what they are until a turn writes them -- rows >= ctx
            //  only, extend_group drops the mark where ctx lies inside the prefix -- and a prefix that is replaced or cleared
            //  takes every mark that speaks of it along, forget_prefix_marks)
            std::fill(b->set_share_.begin(), b->set_share_.begin() + (long)std::min(b->set_share_.size(), (size_t)b->sess_base()), 0);
        }
    };
    struct Rebind {
        TinyLlamaBatch* b; int S; bool done = false;
        void run()
        {
            if (done) return;
            done = true;
            gten_hip_select_stream(0);
            for (int q = 0; q < S; q++) {
                gten_hip_decoder_slot_park(b->dec_, q);
                gten_hip_decoder_slot_bind(b->dec_, q, b->set_kv(q));
            }
        }
        ~Rebind() { run(); }
    };
    // GROUP RECORDS.  One Group per prompt pass whose sets carry a mark: the members that are ready or live, the decoder's
    // record they read from (-1: none yet, or none was free) and the prompt's rows.  The mark travels with the cache set
    // (set_group), as share_mark does; the first member that starts takes a free record and snapshots ITS set's rows into it
    // (the rows are the truth: every member's set holds the same ones), every member then promises its own rows equal it.
    // When the last member has ended the record is released and goes back to the free list.  No mark and no record outlives
    // the queue, however it is left.
    struct Group { int members = 0, rec = -1, rows = 0; bool counted = false; };
    struct GroupRecords {
        TinyLlamaBatch* b;
        std::vector<Group> groups;
        std::vector<int> set_group;                                    // per cache set: its group (-1: no mark)
        std::vector<int> free_rec;
        explicit GroupRecords(TinyLlamaBatch* b_) : b{b_}, set_group((size_t)b_->index_space(), -1)
        {
            const detail::GroupsDecode& h = detail::groups_decode();
            const int cap = (h.set && h.share) ? (b->groups_cap_ < 0 ? TinyLlamaBatch::kGroupsCapDefault : std::min(b->groups_cap_, kGroupsMax)) : 0;
            for (int g = cap - 1; g >= 0; g--) free_rec.push_back(g);
        }
        void mark(int c, int gi) { set_group[(size_t)c] = gi; }
        // slot q was started on set c (kv: its caches): true when it now reads the prompt's chunks from its group's record
        bool start(int q, int c, const gten_hip_kv_ptrs* kv)
        {
            const int gi = set_group[(size_t)c];
            if (gi < 0) return false;
            Group& g = groups[(size_t)gi];
            if (g.rec < 0 && !free_rec.empty()) {
                g.rec = free_rec.back();
                free_rec.pop_back();
                GTEN_HIP_OK(detail::groups_decode().set(b->dec_, g.rec, kv, g.rows));
                b->group_records_now_++;
                if (!g.counted) b->groups_recorded_++;
                g.counted = true;
            }
            if (g.rec < 0) {
                if (!g.counted) b->groups_unrecorded_++;
                g.counted = true;
                return false;
            }
            (void)detail::groups_decode().share(b->dec_, q, g.rec, g.rows);      // (refused, or switched off: the slot decodes on its own copy)
            return true;
        }
        void release(Group& g)
        {
            if (g.rec < 0) return;
            detail::groups_decode().set(b->dec_, g.rec, nullptr, 0);
            free_rec.push_back(g.rec);
            g.rec = -1;
            b->group_records_now_--;
        }
        // the member on set c has ended: the set's mark goes, and with the last member the record
        void leave(int c)
        {
            const int gi = set_group[(size_t)c];
            if (gi < 0) return;
            set_group[(size_t)c] = -1;
            Group& g = groups[(size_t)gi];
            if (--g.members <= 0) release(g);
        }
        ~GroupRecords() { for (Group& g : groups) release(g); }
    };

    // ---- what the queue was given
    TinyLlamaBatch& b_;
    const std::vector<std::vector<int32_t>>& prompts_;
    const int max_tokens_, eos_;
    std::vector<std::vector<int32_t>>& out_;
    const Each<int32_t> max_new_, group_of_, session_;
    Pick& pick_;
    // ---- its state
    const int S_;                                                          // (made first: the decoder and the spare sets exist from here on)
    gten_hip_decoder* const dec_;
    const bool batched_;
    const int slice_;                                                      // (gten_hip_decoder_slot_ids_all reads up to 64 steps at once)
    int lane_rows_, n_lanes_ = 1;
    ServeStats st_;
    std::vector<Slot> slots_;
    // CACHE SETS (round 4).  A prompt is processed onto a free cache set, not onto a free slot: besides the S sets the
    // sequences own there are `spare` more, so that prompts are ready BEFORE the slots that will take them end -- a slot
    // that ends in a harvest gets a ready prompt's set bound (gten_hip_decoder_slot_bind) and joins the very next slice
    // instead of sitting one or two slices out while its replacement is processed.  pool: the free sets; ready: processed
    // prompts waiting for a slot, in queue order.
    std::deque<Ready> ready_;
    std::vector<int> pool_;
    size_t next_ = 0;
    int n_live_ = 0;
    int copies_taken_ = 0;                                                 // items that were copies: a fixed schedule counts prompt passes
    int cnt_ = 0;                                                          // steps of the slice in flight (0: none)
    bool queue_left_ = true;
    bool tail_ = false;                                                    // the queue is empty: the last sequences are kept in as few lanes as they fit
    clock::time_point t_slice_ = clock::now();
    SlotsApply apply_;
    std::vector<int> from_;                                                // harvest's arguments, made once
    std::vector<int32_t> all_ids_;
    // ---- THE GUARDS, last: members are destroyed in reverse order, so however the queue is left -- run() returning or throwing --
    // first every group record is released (~GroupRecords; the slots still stand where they read them), then every slot is parked
    // and bound to its own sequence's set again (~Rebind), and only then does in_serve_ drop and every non-session mark go
    // (~ServeMarks).  The order is part of the behaviour.
    ServeMarks serve_marks_;
    Rebind rebind_;
    GroupRecords group_records_;

    // before any member that speaks to the decoder or counts cache sets is made: the decoder, and the spare sets (returns the slots)
    static int made_ready(TinyLlamaBatch& b)
    {
        b.ensure_decoder();
        b.ensure_spares(b.serve_spares_ >= 0 ? b.serve_spares_ : (b.batched_prompts() ? std::min(b.n_seq() / 4, 64) : 0));
        return b.n_seq();
    }
    bool is_session(int j) const { return session_[j] >= 0; }
    int limit_of(int j) const { return serve_limit((int)prompts_[(size_t)j].size(), max_tokens_, b_.n_ctx_, max_new_[j]); }
    int prompt_len(int j) const
    {
        const int P = (int)prompts_[(size_t)j].size();
        GTEN_ASSERTM(P >= 1 && P <= b_.n_ctx_, "serve: prompt %d has %d ids (context %d)", j, P, b_.n_ctx_);
        return P;
    }

    // a session item has ended: the session takes the out row as its ids (any other item: nothing)
    void session_done(int j)
    {
        const int s = session_[j];
        if (s < 0) return;
        auto& ss = b_.sessions_[(size_t)s];
        const std::vector<int32_t>& row = out_[(size_t)j];
        const int generated = (int)row.size() - (int)prompts_[(size_t)j].size();
        ss.ids = row;
        ss.rows = session_rows_after((int)row.size(), generated);
    }

    // Prompt j has been processed onto cache set `set` and drew first_id.  true: it waits in `ready` for a slot, on that set;
    // false: it ended at once -- an eos (not stored), a first id that entered a final state (kept), or its bound -- and the set
    // stays free (a session takes its row)
    bool admit(int j, int set, int first_id, int limit)
    {
        std::vector<int32_t>& row = out_[(size_t)j];
        st_.admissions++;
        bool goes_on = first_id != eos_;
        if (goes_on) {
            row.push_back(first_id);
            st_.new_tokens++;
            if constexpr (Pick::kFsm) goes_on = !pick_.ended_first(j);
        }
        if (goes_on && (int)row.size() < limit) {
            ready_.push_back(Ready{j, set, (int)row.size(), limit - 1});
            return true;
        }
        session_done(j);
        return false;
    }

    // the next prompt of the queue onto a free cache set (stream 1); false when the queue is empty
    bool prepare_one()
    {
        while (next_ < prompts_.size() && (is_session((int)next_) || !pool_.empty())) {
            const int j = (int)next_++;
            const bool sess = is_session(j);
            std::vector<int32_t>& row = out_[(size_t)j];
            row = prompts_[(size_t)j];
            const int P = prompt_len(j);
            st_.prompt_tokens += P;
            const int limit = limit_of(j);                                 // ids in all
            if (P >= limit) continue;                                      // no room to generate: returned as is
            const auto t0 = clock::now();
            // (a session item on this path -- a conversation under 16 ids, a narrow batch -- is processed whole onto its own set)
            const int c = sess ? b_.sess_base() + session_[j] : pool_.back();
            if (sess) { b_.sess_turns_++; b_.sess_rows_computed_ += (unsigned long long)P; }
            const int best_i = pick_.first(b_, c, row, j);                 // this set's caches now hold rows [0, P) (waits for stream 1 only)
            st_.prefill_s += std::chrono::duration<double>(clock::now() - t0).count();
            if (!admit(j, c, best_i, limit)) continue;                     // ended at once: the set takes the next prompt
            if (!sess) pool_.pop_back();
            return true;
        }
        return next_ < prompts_.size();
    }

    // queue item j as take_batch sees it.  A session item: the rows its plan keeps stay, the others are a continued segment
    // (filled up to 16 rows); where the plan keeps nothing -- a first turn -- or the segment would end past the RoPE table it
    // is a whole prompt
    ServeItem describe(int j)
    {
        ServeItem it;
        it.P = prompt_len(j);
        it.session = is_session(j);
        it.group = it.session ? -1 : group_of_[j];
        if (it.session && b_.continued_prompts()) {
            const auto& ss = b_.sessions_[(size_t)session_[j]];
            SessionPlan pl;
            if (session_plan((int)ss.ids.size(), ss.rows, it.P - (int)ss.ids.size(), true, &pl) && pl.path == kSessionContinued &&
                pl.ctx + pl.seg_rows <= TinyLlamaBatch::kMaxPos) { it.ctx = pl.ctx; it.seg_rows = pl.seg_rows; }
        }
        it.rows = it.ctx > 0 ? it.seg_rows : b_.computed_rows(prompts_[(size_t)j]);   // (a prompt behind the shared prefix: its own rows only)
        it.limit = limit_of(j);
        return it;
    }

    // Wide batches: the next prompts of the queue -- as many as there are free cache sets, kPreMax at most, kPreRows rows in
    // all, `cap` when the schedule is fixed -- as ONE row matrix (prefill_many) on stream 1.  Prompts under 16 ids (and
    // configurations the segmented call does not compute) go one by one through prepare_one().
    // (ITEMS: as many as there are free sets; COMPUTED prompts: kPreMax -- `cap` under a fixed schedule -- and kPreRows rows.
    //  A group's copies cost neither; without sample groups every item is computed and the bounds are the former ones: take_batch)
    bool prepare_batch(int cap)
    {
        if (pool_.empty() && !(next_ < prompts_.size() && is_session((int)next_))) return next_ < prompts_.size();
        const size_t from = next_;
        const ServeBatch t = take_batch(next_, prompts_.size(), (int)pool_.size(), cap, batched_, TinyLlamaBatch::kPreMax, TinyLlamaBatch::kPreRows,
                                        [&](int j) { return describe(j); });
        next_ = t.next;
        for (size_t j = from; j < next_; j++) {
            out_[j] = prompts_[j];
            st_.prompt_tokens += (int64_t)prompts_[j].size();
        }
        const std::vector<int>& js = t.js;
        if (js.empty()) {
            if (next_ >= prompts_.size()) return false;
            const int P = (int)prompts_[next_].size();
            if (batched_ && P >= 16 && P <= TinyLlamaBatch::kPreRows) return true;   // (only prompts without room were taken: look again)
            return prepare_one();
        }
        for (size_t k = 0; k < js.size(); k++) {
            if (!is_session(js[k])) continue;
            const int P = (int)prompts_[(size_t)js[k]].size(), ctx = t.ctx_of[k];
            b_.sess_turns_++; b_.sess_rows_computed_ += (unsigned long long)(P - ctx); b_.sess_rows_kept_ += (unsigned long long)ctx;
            if (ctx > 0) b_.sess_turns_continued_++;
        }
        copies_taken_ += (int)js.size() - t.computed;
        const auto t0 = clock::now();
        std::vector<int> sets, first;
        for (size_t k = 0, taken = 0; k < js.size(); k++)                   // (plain items: the order the sets would be popped in)
            sets.push_back(is_session(js[k]) ? b_.sess_base() + session_[js[k]] : pool_[pool_.size() - 1 - taken++]);
        std::vector<const std::vector<int32_t>*> ps;
        for (int j : js) ps.push_back(&prompts_[(size_t)j]);
        pick_.many(b_, sets, ps, js, &first, t.computed < (int)js.size() ? &t.copy_of : nullptr, t.continued ? &t.ctx_of : nullptr);
        st_.prefill_s += std::chrono::duration<double>(clock::now() - t0).count();
        std::vector<int> unused;
        std::vector<int> readied(js.size(), 0);                              // per computed item: the readied members of its prompt pass
        for (size_t k = 0; k < js.size(); k++) {
            if (admit(js[k], sets[k], first[k], t.limits[k])) readied[t.copy_of[k] < 0 ? k : (size_t)t.copy_of[k]]++;
            else if (!is_session(js[k])) unused.push_back(sets[k]);          // (ended at once: the set stays free)
        }
        mark_groups(t, ps, readied);
        pool_.resize(pool_.size() - (size_t)t.plain);
        for (size_t k = unused.size(); k-- > 0;) pool_.push_back(unused[k]);
        return true;
    }

    // the group mark: at least two readied members behind a prompt of at least one full chunk
    void mark_groups(const ServeBatch& t, const std::vector<const std::vector<int32_t>*>& ps, const std::vector<int>& readied)
    {
        for (size_t k = 0; k < t.js.size(); k++) {
            if (t.copy_of[k] >= 0 || readied[k] < 2 || (int)ps[k]->size() < TinyLlamaBatch::kGroupMinRows) continue;
            const int gi = (int)group_records_.groups.size();
            Group g;
            g.members = readied[k];
            g.rows = (int)ps[k]->size();
            group_records_.groups.push_back(g);
            for (size_t m = k; m < t.js.size(); m++) {
                if (m != k && t.copy_of[m] != (int)k) continue;
                for (const Ready& r : ready_)
                    if (r.j == t.js[m]) group_records_.mark(r.set, gi);    // (readied members only: the others' sets stay free)
            }
        }
    }

    // slot q is over -- its sequence ended, or moves: parked with the others of this batch (apply_), free for the next prompt.
    // What becomes of its cache set is the caller's business, before the call.
    void release_slot(int q)
    {
        apply_.park(q);
        slots_[(size_t)q].set = -1;
        slots_[(size_t)q].job = -1;
        n_live_--;
    }

    // THE TAIL.  Once the queue is empty and nothing waits, the live sequences thin out in every lane alike, and a lane
    // costs a full lane's launches however few of its slots are live.  Whenever they would fit into fewer lanes than they
    // occupy, the sequences of the emptiest lane move: parked here, handed over as ready prompts (their cache sets go
    // with them), started again in the free slots of the lanes that stay -- and the runs of the tail leave empty lanes
    // out (gten_hip_decoder_run_lanes).  Same rows, same ids: a sequence does not know its slot.
    void compact_tail()
    {
        if (!(n_lanes_ > 1 && b_.serve_schedule_ == 0 && !queue_left_ && ready_.empty() && n_live_ > 0)) return;
        std::vector<int> per((size_t)n_lanes_, 0);
        for (int q = 0; q < S_; q++) per[(size_t)(q / lane_rows_)] += slots_[(size_t)q].job >= 0 ? 1 : 0;
        if (const int lane = tail_lane_to_move(per, lane_rows_, n_live_); lane >= 0) {
            apply_.clear();
            for (int q = lane * lane_rows_; q < (lane + 1) * lane_rows_; q++) {
                const Slot s = slots_[(size_t)q];
                if (s.job < 0) continue;
                if constexpr (Pick::kLogprobs) pick_.collect(q, s.job, s.lp_from, s.cur - s.lp_from);
                if constexpr (Pick::kMirostat) pick_.read_mu(q, s.job, s.cur);                          // (the mu its next id is drawn under goes with it)
                ready_.push_back(Ready{s.job, s.set, s.cur, s.last});
                release_slot(q);
            }
            st_.moved += (int64_t)apply_.seq.size();
            apply_.send(dec_);
        }
        tail_ = true;
    }

    // ready prompts take the free slots: bound, started (one slots_apply for all of them), their requests set
    void start_ready()
    {
        apply_.clear();
        if (!ready_.empty()) {
            const std::vector<int> fq = free_slot_order(S_, lane_rows_, n_lanes_, [&](int q) { return slots_[(size_t)q].job < 0; });
            // (the caches of the joining slots were filled on stream 1: the host has waited for that, and the explicit
            //  stream-to-stream dependency makes the next launch on stream 0 acquire what another queue has written)
            if (!fq.empty()) GTEN_HIP_OK(gten_hip_stream_wait(0, 1));
            for (size_t i = 0; i < fq.size() && !ready_.empty(); i++) {
                const int q = fq[i];
                const Ready r = ready_.front();
                ready_.pop_front();
                const std::vector<int32_t>& row = out_[(size_t)r.j];
                GTEN_ASSERTM((int)row.size() == r.cur, "serve: prompt %d holds %zu ids at step %d", r.j, row.size(), r.cur);
                GTEN_HIP_OK(gten_hip_decoder_slot_bind(dec_, q, b_.set_kv(r.set)));
                slots_[(size_t)q] = Slot{r.j, r.cur, r.last, r.set, r.cur};
                // (all joining slots in one call below: their ids, step words and cache-table rows go up behind each other, one wait)
                apply_.join(q, r.cur, r.last, row.data());
                pick_.apply(q, r.j, (int)prompts_[(size_t)r.j].size());                                // (travels with the prompt: also when a sequence moves in the tail)
                if constexpr (Pick::kFsm) pick_.bind_state(q, r.j, r.cur);                              // (... at its current position, with the state the host read)
                if constexpr (Pick::kMirostat) pick_.bind_mu(q, r.j, r.cur);                            // (... and with the mu the host read)
                n_live_++;
            }
        }
        apply_.send(dec_);
        // the joining slots whose sets begin with the shared prefix's rows read them from the decoder's one copy
        // (a group mark wins over a prefix mark on the same set: the whole prompt covers at least as many chunks; also set again
        //  for a sequence that moved in the tail)
        for (const int q : apply_.seq) {
            const int c = slots_[(size_t)q].set;
            if (group_records_.start(q, c, b_.set_kv(c))) continue;
            if (const int P = b_.share_mark(c); P > 0) (void)b_.decoder_share(q, b_.which_mark(c), P);     // (refused: the slot decodes on its own copy, as in prefill_group)
        }
    }

    // ready prompts take the free slots, then the next slice starts (stream 0, asynchronous)
    void launch_slice()
    {
        compact_tail();
        start_ready();
        if (n_live_ == 0) return;
        // (a slot whose run ends inside the slice repeats its last step until the slice is over, slot_start_until: the slice
        //  is cut only when EVERY live slot ends earlier)
        int longest = 0;
        for (const Slot& s : slots_)
            if (s.job >= 0) longest = std::max(longest, s.last - s.cur + 1);
        cnt_ = slice_steps(slice_, longest);
        t_slice_ = clock::now();
        GTEN_HIP_OK(gten_hip_decoder_run_lanes(dec_, cnt_, tail_ ? 1 : 0));
        st_.steps += cnt_;
        int ran = n_lanes_;
        GTEN_HIP_OK(gten_hip_decoder_lane_info(dec_, nullptr, nullptr, &ran));
        st_.lane_steps += (int64_t)cnt_ * ran;
    }

    // the ids of the finished slice; slots that ended are parked (their cache sets are free for the next prompts)
    void harvest()
    {
        // every live slot's ids of the slice in ONE gather + copy (waits for stream 0)
        for (int q = 0; q < S_; q++) from_[(size_t)q] = slots_[(size_t)q].job >= 0 ? slots_[(size_t)q].cur : 0;
        GTEN_HIP_OK(gten_hip_decoder_slot_ids_all(dec_, from_.data(), cnt_, all_ids_.data()));
        apply_.clear();
        for (int q = 0; q < S_; q++) {
            Slot& s = slots_[(size_t)q];
            if (s.job < 0) continue;
            const int got = std::min(cnt_, s.last - s.cur + 1);                                        // (its steps of this slice)
            const int32_t* ids = all_ids_.data() + (size_t)q * (size_t)cnt_;
            std::vector<int32_t>& row = out_[(size_t)s.job];
            bool stop = false;
            const int32_t* entered = nullptr;                                                          // (Pick::kFsm) the state each id entered
            if constexpr (Pick::kFsm) entered = pick_.states(q, s.job, s.cur, got);
            for (int i = 0; i < got && !stop; i++) {
                if (ids[(size_t)i] == eos_) stop = true;
                else {
                    row.push_back(ids[(size_t)i]); st_.new_tokens++;
                    if constexpr (Pick::kFsm)
                        if (entered && pick_.enters_final(s.job, entered[(size_t)i])) stop = true;
                }
            }
            s.cur += got;
            if (stop || s.cur > s.last) {
                // (the records of the ids kept: an eos and what follows it are not stored)
                if constexpr (Pick::kLogprobs) pick_.collect(q, s.job, s.lp_from, (int)row.size() - s.lp_from);
                group_records_.leave(s.set);                                                           // (its group's last member: the record goes back)
                if (s.set >= b_.sess_base()) session_done(s.job);                                      // (a session keeps its set)
                else pool_.push_back(s.set);
                release_slot(q);                                                                       // parked, all of them at once below
            }
        }
        apply_.send(dec_);
        st_.decode_s += std::chrono::duration<double>(clock::now() - t_slice_).count();
        cnt_ = 0;
        GTEN_HIP_OK(gten_hip_stream_wait(1, 0));            // (... and the other way round for the cache sets the parked slots leave)
    }

public:
    ServeQueue(TinyLlamaBatch& b, const std::vector<std::vector<int32_t>>& prompts, int max_tokens, int eos, int slice,
               std::vector<std::vector<int32_t>>* out, Each<int32_t> max_new, Each<int32_t> group_of, Pick& pick, Each<int32_t> session)
        : b_{b}, prompts_{prompts}, max_tokens_{max_tokens}, eos_{eos}, out_{*out}, max_new_{max_new}, group_of_{group_of}, session_{session}, pick_{pick},
          S_{made_ready(b)}, dec_{b.dec_}, batched_{b.batched_prompts()}, slice_{std::min(std::max(slice, 1), 64)}, lane_rows_{S_},
          slots_((size_t)S_), from_((size_t)S_, 0), all_ids_((size_t)S_ * (size_t)slice_), serve_marks_{&b}, rebind_{&b, S_}, group_records_{&b}
    {
        out_.assign(prompts_.size(), {});
        for (int c = b_.n_sets() - 1; c >= 0; c--) pool_.push_back(c);           // (taken from the back: the sequences' own sets first)
        GTEN_HIP_OK(gten_hip_decoder_lane_info(dec_, &lane_rows_, &n_lanes_, nullptr));
        st_.lane_rows = lane_rows_;
        GTEN_HIP_OK(gten_hip_select_stream(0));
        for (int q = 0; q < S_; q++) GTEN_HIP_OK(gten_hip_decoder_slot_park(dec_, q));
    }

    // One host thread: prompts are processed back to back on stream 1; between two prompt calls the slice on stream 0 is
    // polled, and when it has finished its ids are read and the next slice (with the prompts that became ready) starts.
    ServeStats run()
    {
        const int schedule = b_.serve_schedule_;
        int prepared_this_slice = 0;
        for (;;) {
            if (cnt_ > 0) {
                int idle = 0;
                if (schedule > 0) idle = prepared_this_slice >= schedule;   // fixed schedule (tests): k prompts per slice
                else GTEN_HIP_OK(gten_hip_stream_idle(0, &idle));
                // (a session item at the head of the queue needs no free set: it is prepared beside the slice even when every set
                //  is taken.  The other way round, while any set is free prepare_batch may take session items far ahead of the slots
                //  that will run them -- they wait in `ready` on their own sets and hold nothing a plain prompt could use)
                const bool head_is_session = next_ < prompts_.size() && is_session((int)next_);
                if (!idle && queue_left_ && (!pool_.empty() || head_is_session)) {   // slice still running: more prompts beside it
                    GTEN_HIP_OK(gten_hip_select_stream(1));
                    const int before = (int)st_.admissions - copies_taken_;
                    queue_left_ = batched_ ? prepare_batch(schedule > 0 ? schedule - prepared_this_slice : 0) : prepare_one();
                    GTEN_HIP_OK(gten_hip_select_stream(0));
                    prepared_this_slice += batched_ ? std::max(1, (int)st_.admissions - copies_taken_ - before) : 1;
                    continue;
                }
                harvest();                                                  // (waits when nothing is left to prepare)
                prepared_this_slice = 0;
            }
            if (n_live_ == 0 && ready_.empty()) {                           // nothing to decode: a prompt first
                if (!queue_left_ || pool_.empty()) break;                   // queue empty, nothing in flight
                GTEN_HIP_OK(gten_hip_select_stream(1));
                queue_left_ = batched_ ? prepare_batch(schedule) : prepare_one();
                // (with nothing live there is nothing to run beside: prompts are processed -- at the prompt kernels' full rate --
                //  until serve_ramp_ percent of the slots have one, and only then does the first slice start: 669 instead of 709
                //  shared steps on the bench's queue, its first 256 prompts 31.3 k instead of 28.6 k new ids/s; the price is the
                //  first ids' latency, ~0.4 s at full size.  0: the first slice starts with the first batch of prompts)
                while (schedule == 0 && batched_ && queue_left_ && !pool_.empty() && (int)ready_.size() * 100 < S_ * b_.serve_ramp_)
                    queue_left_ = prepare_batch(0);
                GTEN_HIP_OK(gten_hip_select_stream(0));
                if (ready_.empty()) { if (!queue_left_) break; continue; }
            }
            launch_slice();
        }
        // every slot back on its own sequence's caches (all of them are parked now): what follows a serve() -- decode_step,
        // generate -- addresses slot q as sequence q
        for (int q = 0; q < S_; q++) GTEN_HIP_OK(gten_hip_decoder_slot_bind(dec_, q, b_.set_kv(q)));
        rebind_.done = true;
        pick_.clear();                                                      // every slot greedy again, unbound, and nobody asks
        return st_;
    }
};

} // namespace gten

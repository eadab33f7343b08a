// tinyllama_cli.cpp -- command line of the reference (tinyllama.cpp:110-298: options, single prompt or chat loop,
// greedy or top-k sampling) on the HBM-backed gten API of this repository.  SURVEY 8(f) rank 4; host code only -- the
// forward path it drives is libgten_hip.so.  Differences from the reference's main(): no model download step (there is
// no network here: --model PATH, default models/tinyllama.<fp16|q8|q4>.gten as there), --tokenizer PATH (default
// tokenizer.bin), --seed for the top-k sampler, --ids to print token ids instead of text (tests); greedy sampling runs
// with the sampler on the device (host/generate.h); --score PATH prints the log-likelihood of a text file
// (include/gten_host_score.h) instead of generating; --ban / --allow / --min-new constrain the generated ids through bias table 0
// of the model's decoder (include/gten_hip_bias.h), in both generation modes; --logprobs N prints every generated id's log-prob and its N
// most likely alternatives (include/gten_hip_logprobs.h) after the text; --top-p / --min-p cut the top-k draw (include/gten_hip_nucleus.h);
// --repeat-penalty / --frequency-penalty / --presence-penalty / --repeat-last-n penalise the ids already there, in both modes (include/gten_hip_penalty.h);
// --stop / --choice end the answer at, or hold it to, id sequences through a token automaton on the device (include/gten_hip_fsm.h);
// --regex holds it to a regular expression over its text, expanded over the vocabulary on the device (include/gten_hip_regex.h);
// --stop-text ends it at a stop string given as text, a search automaton expanded the same way (include/gten_hip_stoptext.h);
// --json-schema holds it to a JSON schema, compiled to a pattern of --regex's dialect (host/json_schema.h);
// --embed FILE prints one pooled, normalised vector per line of FILE (include/gten_host_embed.h, host/embed.h) instead of generating.
// --ctx-shift lets an answer go on past the window: when it is full the oldest rows behind KEEP are dropped from the K / V caches on the
// device and the rest re-rotated in place (include/gten_hip_shift.h, host/generate_shift.h).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <iterator>
#include <fstream>
#include <iostream>
#include <random>
#include <string>
#include <string_view>
#include <vector>

#include "../../include/gten_hip_regex.h"
#include "../../include/gten_hip_stoptext.h"
#include "embed.h"
#include "fsm_build.h"
#include "json_schema.h"
#include "generate.h"
#include "generate_shift.h"
#include "tokenizer.h"

using namespace gten;

static const char* usage_message = R"(
USAGE:
./tinyllama_cli [options] -p PROMPT  for a single prompt or
./tinyllama_cli [options] for a chat interface.

Optional args.
-f16 :     Use float-16 model and inference (2.2GB). [default]
-q8  :     Use 8-bit quantized model (1.1GB).
-q4  :     Use 4-bit quantized model (0.62GB).
-greedy :  Greedy sampling (argmax on the device) instead of top-k sampling.
--temp T : Temperature to use during sampling. It must be greater than 0. [default=0.9].
--npred  N : Number of tokens to generate. Minimum is 1 and max is 2048. [default=768].
--topk K : Top tokens to randomly select from during prediction. [default=50].
--model PATH :     .gten checkpoint [default=models/tinyllama.<fp16|q8|q4>.gten].
--tokenizer PATH : vocabulary file [default=tokenizer.bin].
--seed S : seed of the top-k sampler [default: random].
--ids :    print token ids instead of text (with --score: one `id logprob rank` line per scored id).
--score PATH : score the text of PATH (plain BPE, no chat template) instead of generating: windows of at most
           --ctx ids, each [1] + the next ctx-1 text ids, so that every text id is scored once.  Prints
           `score: tokens=T nll=<mean -logprob> ppl=<exp(nll)> greedy=<fraction of ids that were the argmax>`.
--ctx N :  window length for --score. Minimum is 17 and max is 2048. [default=2048].
--ban ID[,ID...] :   token ids that are never generated (greedy and top-k alike).
--allow ID[,ID...] : the only token ids that may be generated. With --ban: those of them that are not banned.
--min-new N : --ban / --allow hold for the first N generated ids only; N must be gte 1. [default: for all of them]
--logprobs N : after the text, one line per generated id: `id logprob` and the N most likely ids of its step as `id:logprob`,
           from the unconstrained, untempered logits. N must be gte 0 and lte 20. Combines with --ban / --allow / --min-new.
--top-p F : nucleus sampling: draw from the fewest of the top-k ids whose probability mass reaches F. F must be gt 0 and lte 1.
           [default=1: off]. With --topk 32003: over the whole vocabulary. Not with -greedy or --score.
--min-p F : draw only from ids at least F times as likely as the most likely one. F must be gte 0 and lte 1. [default=0: off].
           Not with -greedy or --score.
--mirostat N : 2: Mirostat v2 sampling (the surprise of the text is held at a target); 0: off; 1 (Mirostat v1) is not implemented. [default=0].
--mirostat-ent F : Mirostat's target surprise tau in bits. F must be gt 0 and lte 32. [default=5.0].
--mirostat-lr F : Mirostat's learning rate eta. F must be gt 0 and lte 1. [default=0.1].
           Not with -greedy, --top-p / --min-p, --score, --embed or the context shift.
--repeat-penalty R : ids the answer or the prompt already holds are made less likely: a positive logit is divided by R, a negative
           one multiplied. R must be gte 0.125 and lte 8. [default=1: off]. Works with -greedy too. Not with --score.
--frequency-penalty F : subtract F from the logit of such an id once per occurrence. |F| must be lte 100. [default=0: off].
--presence-penalty P : subtract P from the logit of such an id once. |P| must be lte 100. [default=0: off].
--repeat-last-n N : the penalties look at the last N ids only; N must be gte 0. [default=0: at all of them]
--stop ID[,ID...] : the answer ends as soon as it ends in this id sequence (which it keeps). Repeatable. Works with -greedy too.
           Not with --choice, --ban, --allow or --score.
--choice ID[,ID...] : the answer is exactly one of the id sequences given this way. Repeatable; none may be a prefix of another.
           Works with -greedy too. Not with --stop, --ban, --allow or --score.
--regex PATTERN : the text of the answer matches PATTERN as a whole (the dialect of host/regex_build.h: literals, classes, groups,
           | ? * + {m,n}, ASCII \d \w \s; no anchors, look-around or back-references). Where the pattern could stop or go on the
           model decides by drawing the end-of-turn id. Works with -greedy too. Not with --choice, --stop, --ban, --allow or
           --score: an answer is bound to one start state of one automaton.
--stop-text STRING : the answer ends as soon as its text holds STRING, wherever in a token it begins or ends; the printed text ends
           before it (--ids prints every id, the one that completes STRING included). Nothing is banned on the way. Repeatable.
           Works with -greedy too. Not with --stop, --choice, --regex, --json-schema, --ban, --allow or --score.
--json-schema FILE : the text of the answer is a JSON document that fits the schema in FILE (types, enum / const, properties /
           required in their order, items with minItems / maxItems, minLength / maxLength, anyOf / oneOf, $ref into $defs; anything
           else that would constrain is refused), compact. The tokenizer's end-of-turn id ends it where it could go on. Works with
           -greedy too. Not with the other automaton flags, --ban, --allow or --score.
--ctx-shift KEEP[,DROP] : go on past the window instead of stopping when it is full: the window is then --ctx positions and --npred may
           exceed it (up to 1048576). Whenever the window is full the first KEEP positions stay, the next DROP are dropped [default:
           half of what lies behind KEEP] and the rest slide down. Works with -greedy, top-k, --top-p / --min-p and the penalties.
           Not with --ban, --allow, --logprobs, --stop, --choice, --regex or --score.
--embed FILE : embed the texts of FILE instead of generating: one text per line (BOS + plain BPE, as --score tokenises; at most --ctx
           ids each), one output line per text: the vector's values as %.9g, separated by blanks. Not with any generation flag
           (-greedy, --temp, --topk, --npred, --seed, -p, --ids and everything above that constrains or samples) or --score.
--pooling mean|last : with --embed: the mean of a text's final-norm rows, or its last row. [default=mean]
--no-normalize : with --embed: print the pooled vector as it is instead of scaling it to length 1.
--layer N : with --embed: the final norm applied to the output of block N (1 .. 22) instead of the last block's. [default=0: the last]
)";

struct Options {
    Dtype model_dtype = kFloat16;
    std::string model_path, tokenizer_path = "tokenizer.bin", prompt, score_path;
    int n_predict = 768, topk = 50, ctx = 2048;
    float temp = 0.9f;
    bool greedy = false, ids = false, seeded = false;
    uint64_t seed = 0;
    std::vector<int32_t> ban, allow;         // --ban / --allow (bias table 0)
    int min_new = 0;
    int logprobs = -1;                       // --logprobs N (-1: off)
    float top_p = 1.f, min_p = 0.f;          // --top-p / --min-p ((1, 0): off)
    int mirostat = 0;                        // --mirostat (0: off; 2: Mirostat v2)
    float miro_tau = 5.f, miro_eta = 0.1f;   // --mirostat-ent / --mirostat-lr
    bool miro_given = false;                 // any of the three flags was given
    bool cut_given = false;
    bool cuts() const { return !(top_p == 1.f && min_p == 0.f); }
    float rep = 1.f, freq = 0.f, pres = 0.f; // --repeat-penalty / --frequency-penalty / --presence-penalty ((1, 0, 0): off)
    int last_n = 0;                          // --repeat-last-n (0: every id so far)
    bool pen_given = false;
    bool penalises() const { return !(rep == 1.f && freq == 0.f && pres == 0.f); }
    bool constrained() const { return !ban.empty() || !allow.empty(); }
    std::vector<std::vector<int32_t>> stop, choice;      // --stop / --choice, one id sequence per flag
    std::string regex;                                   // --regex
    bool regex_given = false;
    std::vector<std::string> stop_text;                  // --stop-text, one string per flag
    bool json_given = false;                             // --json-schema: `regex` holds the schema's pattern
    bool automaton() const { return !stop.empty() || !choice.empty() || regex_given || json_given || !stop_text.empty(); }
    int shift_keep = -1, shift_drop = 0;                 // --ctx-shift KEEP[,DROP] (keep < 0: off)
    bool shifting() const { return shift_keep >= 0; }
    std::string embed_path;                              // --embed FILE
    int pooling = GTEN_HIP_POOL_MEAN, layer = 0;         // --pooling / --layer
    bool normalize = true, embed_flag = false;           // --no-normalize; one of the three given
    bool generation_flag = false;                        // any flag that only generation reads
};

static void emit(const Options& o, Tokenizer& tok, int prev, int id)
{
    if (o.ids) std::cout << id << ' ';
    else std::cerr << tok.decode(prev, id);
}

// "ID[,ID...]" -> ids in [0, n_vocab), none twice; false (with a message) otherwise
static bool parse_id_list(const char* what, const std::string& text, int n_vocab, std::vector<int32_t>* out, bool unique = true)
{
    out->clear();
    size_t pos = 0;
    while (pos <= text.size()) {
        const size_t comma = std::min(text.find(',', pos), text.size());
        const std::string item = text.substr(pos, comma - pos);
        size_t used = 0;
        long v = -1;
        try { v = std::stol(item, &used); } catch (...) { used = 0; }
        if (item.empty() || used != item.size()) { std::cerr << "Invalid " << what << " value: ids are integers separated by commas.\n"; return false; }
        if (v < 0 || v >= n_vocab) { std::cerr << what << " ids must be gte 0 and lt " << n_vocab << ".\n"; return false; }
        if (unique && std::find(out->begin(), out->end(), (int32_t)v) != out->end()) { std::cerr << what << " lists id " << v << " twice.\n"; return false; }
        out->push_back((int32_t)v);
        pos = comma + 1;
    }
    return true;
}

// --ban / --allow as bias table 0 of the model's decoder: allow -> everything else banned, ban -> those ids banned
static void set_constraint(const Options& o, TinyLlama& model)
{
    std::vector<int32_t> ids = o.allow;
    std::vector<float> values(o.allow.size(), 0.f);
    for (const int32_t id : o.ban) {
        const auto it = std::find(ids.begin(), ids.end(), id);
        if (it != ids.end()) values[(size_t)(it - ids.begin())] = -INFINITY;
        else { ids.push_back(id); values.push_back(-INFINITY); }
    }
    const float fill = o.allow.empty() ? 0.f : -INFINITY;
    if (gten_hip_decoder_set_bias_table(model.decoder_handle(), 0, ids.data(), values.data(), (int)ids.size(), fill) != 0) {
        std::cerr << "error: " << gten_hip_last_error() << "\n";
        std::exit(EXIT_FAILURE);
    }
}

// --stop / --choice as the pool of the model's decoder (host/fsm_build.h); the start state the answers are bound to
static int set_automaton(const Options& o, TinyLlama& model, const Tokenizer& tok, int n_vocab)
{
    if (o.regex_given || o.json_given || !o.stop_text.empty()) {
        // the vocabulary's byte strings as decode prints them (control pieces and the ids past the tokenizer: empty), the pattern as a
        // byte automaton, and the expansion of the one over the other on the device
        std::vector<uint8_t> bytes;
        std::vector<int32_t> offsets{0};
        for (int i = 0; i < n_vocab; i++) {
            if (i > 2 && i < tok.vocab_size()) {
                const std::string piece = tok.piece_bytes(i);
                bytes.insert(bytes.end(), piece.begin(), piece.end());
            }
            offsets.push_back((int32_t)bytes.size());
        }
        FsmPool pool(n_vocab);
        int at = -1;
        pool.set_vocab(bytes.data(), offsets.data());
        if (!o.stop_text.empty()) {
            // the strings' Aho-Corasick automaton over bytes as a search range: nothing banned, the id that completes one is final
            std::vector<StopText> strings;
            for (const std::string& t : o.stop_text) strings.push_back(StopText{(const uint8_t*)t.data(), t.size()});
            const int start = pool.add_stop_text(strings.data(), (int)strings.size());
            if (start < 0) {
                std::cerr << "error: --stop-text: the strings do not fit an automaton pool.\n";
                std::exit(EXIT_FAILURE);
            }
            const FsmPool::Regex& r = pool.regex(0);
            const gten_hip_fsm_part_ex part{0, pool.n_states(), nullptr, r.dfa.next.data(), r.dfa.accept.data(), r.dfa.n_states(), -1, GTEN_HIP_FSM_PART_SEARCH};
            if (gten_hip_decoder_set_vocab_bytes(model.decoder_handle(), pool.vocab_bytes(), pool.vocab_offsets()) != 0 ||
                gten_hip_decoder_set_fsm_parts_ex(model.decoder_handle(), pool.n_states(), pool.flags(), &part, 1) != 0) {
                std::cerr << "error: " << gten_hip_last_error() << "\n";
                std::exit(EXIT_FAILURE);
            }
            return start;
        }
        const int start = pool.add_regex(o.regex.c_str(), o.regex.size(), tok.eos, &at);
        if (start < 0) {
            std::cerr << "error: " << (o.json_given ? "--json-schema: " : "--regex: ") << (start == kRegexUnsupported ? "unsupported construct" : start == kRegexTooLarge ? "too many states" : "bad syntax");
            if (at >= 0) std::cerr << " at byte " << at;
            std::cerr << ".\n";
            std::exit(EXIT_FAILURE);
        }
        const FsmPool::Regex& r = pool.regex(0);
        const gten_hip_fsm_part part{0, pool.n_states(), nullptr, r.dfa.next.data(), r.dfa.accept.data(), r.dfa.n_states(), r.eos};
        if (gten_hip_decoder_set_vocab_bytes(model.decoder_handle(), pool.vocab_bytes(), pool.vocab_offsets()) != 0 ||
            gten_hip_decoder_set_fsm_parts(model.decoder_handle(), pool.n_states(), pool.flags(), &part, 1) != 0) {
            std::cerr << "error: " << gten_hip_last_error() << "\n";
            std::exit(EXIT_FAILURE);
        }
        return start;
    }
    const std::vector<std::vector<int32_t>>& lists = o.stop.empty() ? o.choice : o.stop;
    std::vector<int32_t> ids, offsets{0};
    for (const auto& l : lists) {
        ids.insert(ids.end(), l.begin(), l.end());
        offsets.push_back((int32_t)ids.size());
    }
    FsmPool pool(n_vocab);
    const int start = o.stop.empty() ? pool.add_choices(ids.data(), offsets.data(), (int)lists.size()) : pool.add_stop(ids.data(), offsets.data(), (int)lists.size());
    if (start < 0) {
        std::cerr << (start == FsmPool::kPrefix ? "error: a --choice is a prefix of another.\n" : "error: the id sequences do not fit an automaton pool.\n");
        std::exit(EXIT_FAILURE);
    }
    if (gten_hip_decoder_set_fsm(model.decoder_handle(), pool.next(), pool.flags(), pool.n_states()) != 0) {
        std::cerr << "error: " << gten_hip_last_error() << "\n";
        std::exit(EXIT_FAILURE);
    }
    return start;
}

// One answer (host/generate.h).  Plain greedy: the prompt as in the reference, every later id from the device-side argmax, nothing set
// on the decoder.  Top-k (tinyllama.cpp:442-507: the k largest of logits / temp, one draw from their softmax) on the device sampler,
// keyed by (seed, stream = the chat turn, position).  --ban / --allow: either mode under table 0 (top_k 0: greedy over the biased
// logits).  --logprobs: after the ids, one record line per generated id.  --top-p / --min-p: the draw under a cut.  The flow names only
// the stages the options ask for.
static void run(const Options& o, std::string prompt, TinyLlama& model, Tokenizer& tok, uint64_t seed, uint32_t* turn, int fsm_start = -1)
{
    std::vector<int> enc = tok.encode(prompt);
    std::vector<int32_t> tokens(enc.begin(), enc.end());
    const size_t n_prompt = tokens.size(), width = std::max(n_prompt, (size_t)o.n_predict), W = (size_t)std::max(o.logprobs, 0);
    std::vector<float> logprob, top_lp;
    std::vector<int32_t> top_id;
    int rc = 0;
    if (o.shifting()) {
        Request r{o.greedy ? 0 : o.topk, o.temp, seed, (*turn)++, -1, 0, -1, o.top_p, o.min_p, o.rep, o.freq, o.pres, o.last_n, true};
        r.shift_keep = o.shift_keep;
        r.shift_drop = o.shift_drop;
        const char* why = nullptr;
        rc = generate_shifting<kSampled | kBiased | kLogprobs | kNucleus | kPenalty | kFsm>(model, tokens, o.n_predict, tok.eos, r, model.n_ctx_, nullptr, &why);
        if (rc < 0 && why) { std::cerr << "error: " << why << "\n"; std::exit(EXIT_FAILURE); }
    } else if (o.greedy && !o.constrained() && o.logprobs < 0 && !o.penalises() && fsm_start < 0) {
        rc = generate<0>(model, tokens, o.n_predict, tok.eos);
    } else {
        Request r{o.greedy ? 0 : o.topk, o.temp, seed, (*turn)++, o.constrained() ? 0 : -1, o.min_new, o.logprobs, o.top_p, o.min_p,
                  o.rep, o.freq, o.pres, o.last_n, true, fsm_start};
        if (o.mirostat == 2) {
            r.miro_tau = o.miro_tau;
            r.miro_eta = o.miro_eta;
            RecordRows rows;
            if (o.logprobs >= 0) {
                logprob.resize(width);
                top_id.resize(width * W);
                top_lp.resize(width * W);
                rows = RecordRows{logprob.data(), top_id.data(), top_lp.data(), (int)W};
            }
            rc = generate<kSampled | kBiased | kLogprobs | kNucleus | kPenalty | kFsm | kMirostat>(model, tokens, o.n_predict, tok.eos, r, rows);
        } else if (fsm_start >= 0) {
            RecordRows rows;
            if (o.logprobs >= 0) {
                logprob.resize(width);
                top_id.resize(width * W);
                top_lp.resize(width * W);
                rows = RecordRows{logprob.data(), top_id.data(), top_lp.data(), (int)W};
            }
            rc = generate<kSampled | kBiased | kLogprobs | kNucleus | kPenalty | kFsm>(model, tokens, o.n_predict, tok.eos, r, rows);
        } else if (o.penalises()) {
            RecordRows rows;
            if (o.logprobs >= 0) {
                logprob.resize(width);
                top_id.resize(width * W);
                top_lp.resize(width * W);
                rows = RecordRows{logprob.data(), top_id.data(), top_lp.data(), (int)W};
            }
            rc = generate<kSampled | kBiased | kLogprobs | kNucleus | kPenalty>(model, tokens, o.n_predict, tok.eos, r, rows);
        } else if (o.cuts()) {
            RecordRows rows;
            if (o.logprobs >= 0) {
                logprob.resize(width);
                top_id.resize(width * W);
                top_lp.resize(width * W);
                rows = RecordRows{logprob.data(), top_id.data(), top_lp.data(), (int)W};
            }
            rc = generate<kSampled | kBiased | kLogprobs | kNucleus>(model, tokens, o.n_predict, tok.eos, r, rows);
        } else if (o.logprobs >= 0) {
            logprob.resize(width);
            top_id.resize(width * W);
            top_lp.resize(width * W);
            rc = generate<kSampled | kBiased | kLogprobs>(model, tokens, o.n_predict, tok.eos, r, RecordRows{logprob.data(), top_id.data(), top_lp.data(), (int)W});
        } else if (o.constrained()) {
            rc = generate<kSampled | kBiased>(model, tokens, o.n_predict, tok.eos, r);
        } else {
            rc = generate<kSampled>(model, tokens, o.n_predict, tok.eos, r);
        }
    }
    if (rc < 0) {
        std::cerr << "error: " << gten_hip_last_error() << "\n";
        std::exit(EXIT_FAILURE);
    }
    if (!o.stop_text.empty() && !o.ids) {
        // the new text as the search automaton read it (the pieces' bytes), cut before the first stop string
        std::string text;
        for (size_t i = n_prompt; i < tokens.size(); i++)
            if (tokens[i] > 2 && tokens[i] < tok.vocab_size()) text += tok.piece_bytes(tokens[i]);
        std::vector<StopText> strings;
        for (const std::string& t : o.stop_text) strings.push_back(StopText{(const uint8_t*)t.data(), t.size()});
        const StopTextHit hit = stop_text_find(strings.data(), (int)strings.size(), (const uint8_t*)text.data(), (long long)text.size());
        std::cerr << text.substr(0, (size_t)hit.begin);
    } else {
        for (size_t i = n_prompt; i < tokens.size(); i++) emit(o, tok, i == n_prompt ? 1 : tokens[i - 1], tokens[i]);
    }
    (o.ids ? std::cout : std::cerr) << '\n';
    if (o.logprobs < 0) return;
    std::cout.flush();
    for (size_t i = n_prompt; i < tokens.size(); i++) {
        std::printf("%d %.9g", tokens[i], logprob[i]);
        for (size_t a = 0; a < W; a++) std::printf(" %d:%.9g", top_id[i * W + a], top_lp[i * W + a]);
        std::printf("\n");
    }
    std::fflush(stdout);
}

// --score: the file's plain BPE ids in windows [1] + up to ctx - 1 text ids, all windows through score_many (BOS is context
// only: every text id is scored exactly once, against the logits of the row before it)
static int run_score(const Options& o, TinyLlama& model, Tokenizer& tok)
{
    std::ifstream f{o.score_path, std::ios::binary};
    if (!f.is_open()) { std::cerr << "error: cannot open " << o.score_path << ".\n"; return EXIT_FAILURE; }
    const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const std::vector<int> ids = tok.encode_plain(text);
    std::vector<int32_t> tokens, targets, starts{0};
    for (size_t i = 0; i < ids.size(); i += (size_t)o.ctx - 1) {
        const size_t take = std::min(ids.size() - i, (size_t)o.ctx - 1);
        tokens.push_back(1);
        tokens.insert(tokens.end(), ids.begin() + (long)i, ids.begin() + (long)(i + take));
        targets.insert(targets.end(), ids.begin() + (long)i, ids.begin() + (long)(i + take));
        targets.push_back(-1);
        starts.push_back((int32_t)tokens.size());
    }
    const int T = (int)ids.size();
    double nll = 0.0;
    int greedy = 0;
    if (T > 0) {
        std::vector<float> lp(tokens.size());
        std::vector<int32_t> rank(tokens.size());
        model.score_many(tokens.data(), starts.data(), (int)starts.size() - 1, targets.data(), lp.data(), rank.data());
        for (size_t i = 0; i < tokens.size(); i++) {
            if (targets[i] < 0) continue;
            nll -= lp[i];
            greedy += rank[i] == 0;
            if (o.ids) std::printf("%d %.9g %d\n", targets[i], lp[i], rank[i]);
        }
        nll /= T;
    }
    std::printf("score: tokens=%d nll=%.9g ppl=%.9g greedy=%.9g\n", T, nll, std::exp(nll), T > 0 ? (double)greedy / T : 0.0);
    return 0;
}

// --embed: one text per line as [1] + its plain BPE ids, all of them through embed_many (host/embed.h), one line of values per text
static int run_embed(const Options& o, TinyLlama& model, Tokenizer& tok)
{
    std::ifstream f{o.embed_path, std::ios::binary};
    if (!f.is_open()) { std::cerr << "error: cannot open " << o.embed_path << ".\n"; return EXIT_FAILURE; }
    std::vector<int32_t> tokens, starts{0};
    std::string line;
    while (std::getline(f, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        const std::vector<int> ids = tok.encode_plain(line);
        tokens.push_back(1);
        tokens.insert(tokens.end(), ids.begin(), ids.end());
        starts.push_back((int32_t)tokens.size());
    }
    const int n_texts = (int)starts.size() - 1;
    std::vector<int> lengths;
    if (const char* why = embed_texts_ok(model, tokens.data(), starts.data(), n_texts, o.layer, &lengths)) {
        std::cerr << "--embed: " << why << " (--ctx " << o.ctx << ").\n";
        return EXIT_FAILURE;
    }
    const size_t E = (size_t)model.params.n_embd;
    std::vector<float> out((size_t)n_texts * E);
    embed_many(model, tokens.data(), starts.data(), lengths, o.pooling, o.normalize, o.layer, out.data());
    for (int k = 0; k < n_texts; k++) {
        for (size_t c = 0; c < E; c++) std::printf(c ? " %.9g" : "%.9g", out[(size_t)k * E + c]);
        std::printf("\n");
    }
    std::fflush(stdout);
    return 0;
}

int main(int argc, char const* argv[])
{
    Options o;
    std::string model_id = "fp16";
    for (int i = 1; i < argc; i++) {
        const std::string_view arg{argv[i]};
        auto value = [&](const char* what) -> const char* {
            if (i + 1 >= argc) { std::cerr << what << " value is missing.\n"; std::exit(EXIT_FAILURE); }
            return argv[++i];
        };
        if (arg == "--help" || arg == "-h") { std::cout << usage_message << "\n"; return 0; }
        else if (arg == "-f16") { o.model_dtype = kFloat16; model_id = "fp16"; }
        else if (arg == "-q8") { o.model_dtype = kQint8; model_id = "q8"; }
        else if (arg == "-q4") { o.model_dtype = kQint4; model_id = "q4"; }
        else if (arg == "-greedy") o.greedy = true;
        else if (arg == "--ids") o.ids = true;
        else if (arg == "-p") o.prompt = value("prompt");
        else if (arg == "--model") o.model_path = value("model");
        else if (arg == "--tokenizer") o.tokenizer_path = value("tokenizer");
        else if (arg == "--score") o.score_path = value("score");
        else if (arg == "--embed") o.embed_path = value("embed");
        else if (arg == "--pooling") {
            const std::string v = value("pooling");
            if (v != "mean" && v != "last") { std::cerr << "pooling must be mean or last.\n"; return -1; }
            o.pooling = v == "mean" ? GTEN_HIP_POOL_MEAN : GTEN_HIP_POOL_LAST;
            o.embed_flag = true;
        }
        else if (arg == "--no-normalize") { o.normalize = false; o.embed_flag = true; }
        else if (arg == "--layer") {
            int v = -1;
            try { v = std::stoi(value("layer")); } catch (...) { std::cerr << "Invalid layer value.\n"; return -1; }
            if (v < 0 || v > 22) { std::cerr << "layer must be gte 0 and lte 22.\n"; return -1; }
            o.layer = v;
            o.embed_flag = true;
        }
        else if (arg == "--ctx") {
            int v = 0;
            try { v = std::stoi(value("ctx")); } catch (...) { std::cerr << "Invalid ctx value.\n"; return -1; }
            if (v < 17 || v > 2048) { std::cerr << "ctx must be gte 17 and lte 2048.\n"; return -1; }
            o.ctx = v;
        }
        else if (arg == "--seed") { o.seed = std::strtoull(value("seed"), nullptr, 10); o.seeded = true; }
        else if (arg == "--npred") {
            int v = 0;
            try { v = std::stoi(value("npred")); } catch (...) { std::cerr << "Invalid npred value.\n"; return -1; }
            if (v < 1 || v > (1 << 20)) { std::cerr << "npred must be greater than 1 and less than 2048.\n"; return -1; }
            o.n_predict = v;
            o.generation_flag = true;
        } else if (arg == "--temp") {
            float v = 0.f;
            try { v = std::stof(value("temp")); } catch (...) { std::cerr << "Invalid temp value \n"; return -1; }
            if (v <= 0.0f) { std::cerr << "temp value must be greater than zero.\n"; return -1; }
            o.temp = v;
            o.generation_flag = true;
        } else if (arg == "--topk") {
            int v = 0;
            try { v = std::stoi(value("topk")); } catch (...) { std::cerr << "Invalid topk value.\n"; return -1; }
            if (v < 1 || v > 32003) { std::cerr << "topk must be gte 1 and lte " << 32003 << ".\n"; return -1; }
            o.topk = v;
            o.generation_flag = true;
        } else if (arg == "--ban") {
            if (!parse_id_list("ban", value("ban"), 32003, &o.ban)) return -1;
        } else if (arg == "--allow") {
            if (!parse_id_list("allow", value("allow"), 32003, &o.allow)) return -1;
        } else if (arg == "--min-new") {
            int v = 0;
            try { v = std::stoi(value("min-new")); } catch (...) { std::cerr << "Invalid min-new value.\n"; return -1; }
            if (v < 1 || v > 2048) { std::cerr << "min-new must be gte 1 and lte 2048.\n"; return -1; }
            o.min_new = v;
        } else if (arg == "--logprobs") {
            const std::string text = value("logprobs");
            size_t used = 0;
            int v = -1;
            try { v = std::stoi(text, &used); } catch (...) { used = 0; }
            if (text.empty() || used != text.size()) { std::cerr << "Invalid logprobs value.\n"; return -1; }
            if (v < 0 || v > GTEN_HIP_LOGPROBS_TOP) { std::cerr << "logprobs must be gte 0 and lte " << GTEN_HIP_LOGPROBS_TOP << ".\n"; return -1; }
            o.logprobs = v;
        } else if (arg == "--mirostat") {
            const std::string text = value("mirostat");
            size_t used = 0;
            int v = -1;
            try { v = std::stoi(text, &used); } catch (...) { used = 0; }
            if (text.empty() || used != text.size()) { std::cerr << "Invalid mirostat value.\n"; return -1; }
            if (v == 1) { std::cerr << "mirostat 1 (Mirostat v1) is not implemented: use --mirostat 2.\n"; return -1; }
            if (v != 0 && v != 2) { std::cerr << "mirostat must be 0 or 2.\n"; return -1; }
            o.mirostat = v;
            o.miro_given = true;
        } else if (arg == "--mirostat-ent" || arg == "--mirostat-lr") {
            const bool is_ent = arg == "--mirostat-ent";
            const char* name = is_ent ? "mirostat-ent" : "mirostat-lr";
            const std::string text = value(name);
            size_t used = 0;
            float v = -1.f;
            try { v = std::stof(text, &used); } catch (...) { used = 0; }
            if (text.empty() || used != text.size() || !std::isfinite(v)) { std::cerr << "Invalid " << name << " value.\n"; return -1; }
            if (is_ent) {
                if (!(v > 0.f && v <= 32.f)) { std::cerr << "mirostat-ent must be gt 0 and lte 32.\n"; return -1; }
                o.miro_tau = v;
            } else {
                if (!(v > 0.f && v <= 1.f)) { std::cerr << "mirostat-lr must be gt 0 and lte 1.\n"; return -1; }
                o.miro_eta = v;
            }
            o.miro_given = true;
        } else if (arg == "--top-p" || arg == "--min-p") {
            const bool is_top = arg == "--top-p";
            const char* name = is_top ? "top-p" : "min-p";
            const std::string text = value(name);
            size_t used = 0;
            float v = -1.f;
            try { v = std::stof(text, &used); } catch (...) { used = 0; }
            if (text.empty() || used != text.size() || !std::isfinite(v)) { std::cerr << "Invalid " << name << " value.\n"; return -1; }
            if (is_top) {
                if (!(v > 0.f && v <= 1.f)) { std::cerr << "top-p must be gt 0 and lte 1.\n"; return -1; }
                o.top_p = v;
            } else {
                if (!(v >= 0.f && v <= 1.f)) { std::cerr << "min-p must be gte 0 and lte 1.\n"; return -1; }
                o.min_p = v;
            }
            o.cut_given = true;
        } else if (arg == "--repeat-penalty" || arg == "--frequency-penalty" || arg == "--presence-penalty") {
            const char* name = arg == "--repeat-penalty" ? "repeat-penalty" : arg == "--frequency-penalty" ? "frequency-penalty" : "presence-penalty";
            const std::string text = value(name);
            size_t used = 0;
            float v = 0.f;
            try { v = std::stof(text, &used); } catch (...) { used = 0; }
            if (text.empty() || used != text.size() || !std::isfinite(v)) { std::cerr << "Invalid " << name << " value.\n"; return -1; }
            if (arg == "--repeat-penalty") {
                if (!(v >= GTEN_HIP_PENALTY_R_MIN && v <= GTEN_HIP_PENALTY_R_MAX)) { std::cerr << "repeat-penalty must be gte 0.125 and lte 8.\n"; return -1; }
                o.rep = v;
            } else {
                if (!(std::fabs(v) <= GTEN_HIP_PENALTY_ADD_MAX)) { std::cerr << name << " must be gte -100 and lte 100.\n"; return -1; }
                (arg == "--frequency-penalty" ? o.freq : o.pres) = v;
            }
            o.pen_given = true;
        } else if (arg == "--repeat-last-n") {
            const std::string text = value("repeat-last-n");
            size_t used = 0;
            int v = -1;
            try { v = std::stoi(text, &used); } catch (...) { used = 0; }
            if (text.empty() || used != text.size()) { std::cerr << "Invalid repeat-last-n value.\n"; return -1; }
            if (v < 0) { std::cerr << "repeat-last-n must be gte 0.\n"; return -1; }
            o.last_n = v;
            o.pen_given = true;
        } else if (arg == "--stop" || arg == "--choice") {
            const bool is_stop = arg == "--stop";
            std::vector<int32_t> list;
            if (!parse_id_list(is_stop ? "stop" : "choice", value(is_stop ? "stop" : "choice"), 32003, &list, false)) return -1;
            (is_stop ? o.stop : o.choice).push_back(list);
        } else if (arg == "--ctx-shift") {
            std::vector<int32_t> pair;
            if (!parse_id_list("ctx-shift", value("ctx-shift"), 2048, &pair, false)) return -1;
            if (pair.size() > 2 || (pair.size() == 2 && pair[1] < 1)) { std::cerr << "ctx-shift takes KEEP or KEEP,DROP with DROP gte 1.\n"; return -1; }
            o.shift_keep = pair[0];
            o.shift_drop = pair.size() == 2 ? pair[1] : 0;
        } else if (arg == "--regex") {
            o.regex = value("regex");
            o.regex_given = true;
            int at = -1;
            ByteDfa dfa;
            if (const int rc = regex_compile(o.regex.c_str(), o.regex.size(), dfa, &at)) {
                std::cerr << "--regex: " << (rc == kRegexUnsupported ? "unsupported construct" : rc == kRegexTooLarge ? "too many states" : "bad syntax");
                if (at >= 0) std::cerr << " at byte " << at;
                std::cerr << ".\n";
                return -1;
            }
        } else if (arg == "--stop-text") {
            const std::string text = value("stop-text");
            if (text.empty()) { std::cerr << "--stop-text: an empty string.\n"; return -1; }
            o.stop_text.push_back(text);
        } else if (arg == "--json-schema") {
            const std::string path = value("json-schema");
            std::ifstream sf{path, std::ios::binary};
            if (!sf.is_open()) { std::cerr << "--json-schema: cannot read " << path << ".\n"; return -1; }
            const std::string schema((std::istreambuf_iterator<char>(sf)), std::istreambuf_iterator<char>());
            std::string error;
            if (const int rc = json_schema_regex(schema.data(), schema.size(), 0, 2, o.regex, error)) {
                if (rc == kJsonUnsupported) std::cerr << "--json-schema: unsupported: " << error << ".\n";
                else std::cerr << "--json-schema: malformed JSON at byte " << error << ".\n";
                return -1;
            }
            ByteDfa dfa;
            if (const int rc = regex_compile(o.regex.c_str(), o.regex.size(), dfa, nullptr)) {
                std::cerr << "--json-schema: " << (rc == kRegexTooLarge ? "too many states" : "the schema's pattern is refused") << ".\n";
                return -1;
            }
            o.json_given = true;
        } else {
            std::cerr << "error: Unknown argument: " << arg << "\n" << usage_message;
            return EXIT_FAILURE;
        }
    }
    if (o.embed_flag && o.embed_path.empty()) { std::cerr << "--pooling, --no-normalize and --layer need --embed.\n"; return -1; }
    if (!o.embed_path.empty() && (o.generation_flag || o.greedy || o.ids || o.seeded || !o.prompt.empty() || o.constrained() || o.min_new > 0 || o.logprobs >= 0 ||
                                  o.cut_given || o.miro_given || o.pen_given || o.last_n > 0 || o.automaton() || o.shifting() || !o.score_path.empty())) {
        std::cerr << "--embed does not generate: it does not combine with -p, --score, --ids, -greedy or any flag that samples, constrains or extends generation.\n";
        return -1;
    }
    if (!o.shifting() && o.n_predict > 2048) { std::cerr << "npred must be greater than 1 and less than 2048.\n"; return -1; }
    if (o.shifting() && (o.constrained() || o.logprobs >= 0 || o.automaton() || !o.score_path.empty())) {
        std::cerr << "--ctx-shift does not combine with --ban, --allow, --logprobs, --stop, --choice, --regex or --score: what they bind by position is not carried through a shift.\n";
        return -1;
    }
    if (o.shifting() && !shift_ok(o.ctx, o.shift_keep, o.shift_drop)) { std::cerr << "ctx-shift: KEEP + DROP do not fit the window of " << o.ctx << " positions.\n"; return -1; }
    if (o.mirostat == 2 && o.greedy) { std::cerr << "mirostat needs top-k sampling: not with -greedy.\n"; return -1; }
    if (o.mirostat == 2 && o.cut_given) { std::cerr << "mirostat and top-p / min-p do not compose: give one of them.\n"; return -1; }
    if (o.miro_given && !o.score_path.empty()) { std::cerr << "mirostat does not apply to --score.\n"; return -1; }
    if (o.mirostat == 2 && o.shifting()) { std::cerr << "mirostat does not work with the context shift yet.\n"; return -1; }
    if (o.cut_given && o.greedy) { std::cerr << "top-p and min-p need top-k sampling: not with -greedy.\n"; return -1; }
    if (o.cut_given && !o.score_path.empty()) { std::cerr << "top-p and min-p do not apply to --score.\n"; return -1; }
    if (o.pen_given && !o.score_path.empty()) { std::cerr << "the repeat, frequency and presence penalties do not apply to --score.\n"; return -1; }
    if (!o.stop.empty() && !o.choice.empty()) { std::cerr << "--stop and --choice do not combine: an answer follows one automaton.\n"; return -1; }
    if (o.regex_given && !o.choice.empty()) { std::cerr << "--regex and --choice do not combine: an answer follows one automaton.\n"; return -1; }
    if (o.regex_given && !o.stop.empty()) { std::cerr << "--regex and --stop do not combine: an answer is bound to one start state.\n"; return -1; }
    for (const char* other : {"--stop", "--choice", "--regex", "--stop-text"}) {
        const std::string name = other;
        const bool given = name == "--stop" ? !o.stop.empty() : name == "--choice" ? !o.choice.empty() : name == "--regex" ? o.regex_given : !o.stop_text.empty();
        if (o.json_given && given) { std::cerr << "--json-schema and " << name << " do not combine: an answer is bound to one start state of one automaton.\n"; return -1; }
        if (!o.stop_text.empty() && given && name != "--stop-text") {
            std::cerr << "--stop-text and " << name << " do not combine: an answer is bound to one start state of one automaton.\n";
            return -1;
        }
    }
    if (o.automaton() && o.constrained()) { std::cerr << "--stop, --choice and --regex do not combine with --ban or --allow.\n"; return -1; }
    if (o.automaton() && !o.score_path.empty()) { std::cerr << "--stop, --choice and --regex do not apply to --score.\n"; return -1; }
    for (size_t a = 0; a < o.choice.size(); a++)
        for (size_t b = 0; b < o.choice.size(); b++)
            if (a != b && o.choice[a].size() <= o.choice[b].size() && std::equal(o.choice[a].begin(), o.choice[a].end(), o.choice[b].begin())) {
                std::cerr << "a --choice is a prefix of another.\n";
                return -1;
            }
    if (o.min_new > 0 && !o.constrained()) { std::cerr << "min-new needs --ban or --allow.\n"; return -1; }
    if (!o.allow.empty() && std::all_of(o.allow.begin(), o.allow.end(), [&](int32_t id) { return std::find(o.ban.begin(), o.ban.end(), id) != o.ban.end(); })) {
        std::cerr << "--ban bans every id of --allow.\n";
        return -1;
    }
    if (o.model_path.empty()) o.model_path = "models/tinyllama." + model_id + ".gten";

    std::ifstream checkpoint{o.model_path, std::ios::binary};
    if (!checkpoint.is_open()) {
        std::cerr << "error: cannot open the checkpoint " << o.model_path << " (convert one with `python -m tinyllama.cpp_amd.convert`).\n";
        return EXIT_FAILURE;
    }
    {
        std::ifstream vf{o.tokenizer_path, std::ios::binary};
        if (!vf.is_open()) { std::cerr << "error: cannot open the vocabulary file " << o.tokenizer_path << ".\n"; return EXIT_FAILURE; }
    }
    ModuleDtype dtype;
    dtype.wdtype = o.model_dtype;
    dtype.adtype = (o.model_dtype == kFloat16) ? kFloat16 : kQint8;          // tinyllama.cpp:258-265

    TinyLlama model{o.score_path.empty() && o.embed_path.empty() && !o.shifting() ? o.n_predict : o.ctx, dtype};
    model.load_from_ckpt(checkpoint);
    Tokenizer tokenizer{o.tokenizer_path.c_str(), 32000};
    if (!o.score_path.empty()) return run_score(o, model, tokenizer);
    if (!o.embed_path.empty()) return run_embed(o, model, tokenizer);

    uint64_t seed = o.seed;
    if (!o.seeded) {
        std::random_device rd;
        seed = ((uint64_t)rd() << 32) | (uint64_t)rd();
    }
    if (o.constrained()) set_constraint(o, model);
    const int fsm_start = o.automaton() ? set_automaton(o, model, tokenizer, 32003) : -1;
    uint32_t turn = 0;
    auto answer = [&](const std::string& prompt) { run(o, prompt, model, tokenizer, seed, &turn, fsm_start); };
    if (o.prompt.empty()) {
        std::cout << "Chat interface. Write your prompt and press enter to submit. Enter q or press ctrl+c to quit.\n";
        std::string prompt;
        while (true) {
            std::cerr << "\n\n[You]: ";
            if (!std::getline(std::cin, prompt) || prompt == "q") break;
            std::cerr << "\n[Tinyllama-Chat]: \n\n";
            answer(prompt);
        }
    } else {
        answer(o.prompt);
    }
    return 0;
}

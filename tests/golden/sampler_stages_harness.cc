// sampler_stages_harness.cc -- drives the reference's own sample_* functions (llm/src/Generate.cc, compiled next to this file by make_sampler_stages_golden.py into a
// temporary directory) in the order LLaMA3Generate.cc:151-179 calls them -- top-k, tail-free, typical, top-p, temperature, the token's softmax -- and records the
// candidates after every stage: the size, the ids in their current order, and p as the stage left it.  No sampling arithmetic lives here.
//
//   in : int32 rows, vocab, k, nrecent; float top_p, temp, repeat_penalty, alpha_frequency, alpha_presence, tfs_z, typical_p; then per row float logits[vocab],
//        int32 recent[nrecent]
//   out: per row int32 greedy, n_tfs, n_typ, n; int32 ids[k]; float logit[k], p[k] (behind top-k: the softmax over the k); int32 ids_typ[k]; float p_typ[k] (behind
//        typical: n_typ entries in the order it left; -1 / 0 behind them); float p_top[k] (the softmax top-p walked, n_typ entries); float final_p[k] (n entries)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "Generate.h"

static void must(bool ok, const char *what) {
    if (!ok) {
        fprintf(stderr, "sampler_stages_harness: %s\n", what);
        exit(1);
    }
}

int main(int argc, char **argv) {
    must(argc == 3, "usage: sampler_stages_harness IN OUT");
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    must(in && out, "cannot open files");
    int hdr[4];
    float par[7];
    must(fread(hdr, 4, 4, in) == 4 && fread(par, 4, 7, in) == 7, "short header");
    const int rows = hdr[0], vocab = hdr[1], k = hdr[2], nrecent = hdr[3];
    const float top_p = par[0], temp = par[1], repeat_penalty = par[2], alpha_frequency = par[3], alpha_presence = par[4], tfs_z = par[5], typical_p = par[6];
    must(temp > 0, "the stages run in the temperature branch only");
    std::vector<float> logits(vocab);
    std::vector<int> recent(nrecent);
    for (int r = 0; r < rows; ++r) {
        must(fread(logits.data(), 4, vocab, in) == (size_t)vocab && fread(recent.data(), 4, nrecent, in) == (size_t)nrecent, "short row");
        std::vector<OPT_token_data> cand;
        cand.reserve(vocab);
        for (int id = 0; id < vocab; ++id) cand.push_back(OPT_token_data{id, logits[id], 0.0f});
        OPT_token_data_array arr = {cand.data(), cand.size(), false};
        sample_repetition_penalty(&arr, recent.data(), nrecent, repeat_penalty);
        sample_frequency_and_presence_penalties(&arr, recent.data(), nrecent, alpha_frequency, alpha_presence);
        const int greedy = sample_token_greedy(&arr);
        std::vector<int> ids(k, -1), ids_typ(k, -1);
        std::vector<float> lg(k, 0.f), p(k, 0.f), p_typ(k, 0.f), p_top(k, 0.f), fp(k, 0.f);
        sample_top_k(&arr, k, 1);
        must((int)arr.size == k, "top-k left another count");
        sample_softmax(&arr);  // what sample_tail_free computes first; recorded here because tfs_z >= 1 returns before it (p only: the later stages compute their own)
        for (int i = 0; i < k; ++i) {
            ids[i] = arr.data[i].id;
            lg[i] = arr.data[i].logit;
            p[i] = arr.data[i].p;
        }
        sample_tail_free(&arr, tfs_z, 1);
        const int n_tfs = (int)arr.size;
        sample_typical(&arr, typical_p, 1);
        const int n_typ = (int)arr.size;
        for (int i = 0; i < n_typ; ++i) {
            ids_typ[i] = arr.data[i].id;
            p_typ[i] = arr.data[i].p;
        }
        sample_softmax(&arr);  // what sample_top_p computes first; recorded here because top_p >= 1 returns before it
        for (int i = 0; i < n_typ; ++i) p_top[i] = arr.data[i].p;
        sample_top_p(&arr, top_p, 1);
        const int n = (int)arr.size;
        sample_temperature(&arr, temp);
        sample_softmax(&arr);  // sample_token's first statement; the draw itself (std::discrete_distribution on mt19937) is not recorded
        for (int i = 0; i < n; ++i) fp[i] = arr.data[i].p;
        const int head[4] = {greedy, n_tfs, n_typ, n};
        fwrite(head, 4, 4, out);
        fwrite(ids.data(), 4, k, out);
        fwrite(lg.data(), 4, k, out);
        fwrite(p.data(), 4, k, out);
        fwrite(ids_typ.data(), 4, k, out);
        fwrite(p_typ.data(), 4, k, out);
        fwrite(p_top.data(), 4, k, out);
        fwrite(fp.data(), 4, k, out);
    }
    fclose(in);
    must(fclose(out) == 0, "write failed");
    return 0;
}

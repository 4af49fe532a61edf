// mirostat_harness.cc -- drives the reference's own sample_* functions (llm/src/Generate.cc, compiled next to this file by make_mirostat_golden.py into a temporary
// directory) in the order LLaMA3Generate.cc:151-171 calls them in its mirostat branches -- the two penalties, then sample_temperature and sample_token_mirostat[_v2] --
// with sample_top_k(k, 1) between the penalties and the temperature: the device rule's universe is the row's top-k candidates (with vocab <= k it removes nothing and
// the chain is the reference's own).  mu is carried from row to row, as the reference's function-static is.  No sampling arithmetic lives here: s_hat and k are locals
// of sample_token_mirostat and cannot be recorded; the count it keeps can (candidates->size behind the call).
//
//   in : int32 rows, vocab, k, nrecent, mode, m; float temp, repeat_penalty, alpha_frequency, alpha_presence, tau, eta; then per row float logits[vocab],
//        int32 recent[nrecent]
//   out: per row float mu_in; int32 ids[k]; float logit[k] (behind top-k: the sorted penalised logits, before the division), p[k] (the softmax over logit / temp);
//        int32 kept; float final_p[k] (kept entries, 0 behind); int32 X (the token the reference drew); float mu_out
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "Generate.h"

static void must(bool ok, const char *what) {
    if (!ok) {
        fprintf(stderr, "mirostat_harness: %s\n", what);
        exit(1);
    }
}

int main(int argc, char **argv) {
    must(argc == 3, "usage: mirostat_harness IN OUT");
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    must(in && out, "cannot open files");
    int hdr[6];
    float par[6];
    must(fread(hdr, 4, 6, in) == 6 && fread(par, 4, 6, in) == 6, "short header");
    const int rows = hdr[0], vocab = hdr[1], k = hdr[2], nrecent = hdr[3], mode = hdr[4], m = hdr[5];
    const float temp = par[0], repeat_penalty = par[1], alpha_frequency = par[2], alpha_presence = par[3], tau = par[4], eta = par[5];
    must(temp > 0 && (mode == 1 || mode == 2) && k <= vocab, "mirostat runs in the temperature branch; mode 1 or 2; k <= vocab");
    float mu = 2.0f * tau;  // LLaMA3Generate.cc:163, :169
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
        sample_top_k(&arr, k, 1);
        must((int)arr.size == k, "top-k left another count");
        std::vector<int> ids(k, -1);
        std::vector<float> lg(k, 0.f), p(k, 0.f), fp(k, 0.f);
        for (int i = 0; i < k; ++i) {
            ids[i] = arr.data[i].id;
            lg[i] = arr.data[i].logit;
        }
        sample_temperature(&arr, temp);
        sample_softmax(&arr);  // sample_token_mirostat[_v2]'s first statement, recorded here because the function goes on to cut
        for (int i = 0; i < k; ++i) p[i] = arr.data[i].p;
        const float mu_in = mu;
        const int X = mode == 1 ? sample_token_mirostat(vocab, &arr, tau, eta, m, &mu) : sample_token_mirostat_v2(&arr, tau, eta, &mu);
        const int kept = (int)arr.size;
        must(kept >= 1 && kept <= k, "the reference cut to an empty or a longer list (choose mu / tau so that it does not)");
        for (int i = 0; i < kept; ++i) fp[i] = arr.data[i].p;
        fwrite(&mu_in, 4, 1, out);
        fwrite(ids.data(), 4, k, out);
        fwrite(lg.data(), 4, k, out);
        fwrite(p.data(), 4, k, out);
        fwrite(&kept, 4, 1, out);
        fwrite(fp.data(), 4, k, out);
        fwrite(&X, 4, 1, out);
        fwrite(&mu, 4, 1, out);
    }
    fclose(in);
    must(fclose(out) == 0, "write failed");
    return 0;
}

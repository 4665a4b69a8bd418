// nd_handle.hpp -- the ensemble handle as its two translation units see it: nd_handle.hip builds and loads it, nd_sampler.hip runs it.
// Private to those two; the public face is include/nested_diffusion.h.
#pragma once
#include "nd_frag.hpp"
#include "nd_skinny.hpp"
#include "nd_step.hpp"
#include "nd_host.hpp"

#include <map>
#include <tuple>
#include <vector>

#define ND_KEEP_BYTES 208.0e6     // weights kept Infinity-Cache resident across steps (see nd_load_member)
// L_LIN2S / L_LIN3S: the two step blocks with frag32b3 operands (bf16 matrix pipe, exact fp32 products: rows > 128 only)
enum { L_ENC0 = 0, L_ENC1 = 1, L_ENC2 = 2, L_LIN2 = 3, L_LIN3 = 4, L_LIN2S = 5, L_LIN3S = 6, L_COUNT = 7 };

struct MemberHost {
    bool loaded = false;
    float *sc0, *sh0, *sc1, *sh1, *sc2, *sh2;
    float *A[3], *Cc[3];
    float *w_enc0, *w_enc3, *w_enc6, *w_lin2, *w_lin3;   // frag16-packed weights
    float *w_lin1, *w_lin4, *b_lin4;                      // small row-major copies
    float *e0, *e1, *xe, *ybuf, *h1, *h2, *epart, *splitk;
    void *w_lin2s = nullptr, *w_lin3s = nullptr, *h1s = nullptr, *h2s = nullptr;   // frag32b3 images (handles with max_rows > 128, fp32)
    bool h_split = false;        // which copies of h1 / h2 the LAST launch over this member wrote: the frag32b3 images (true) or h1 / h2 (nd_member_buffer)
};

struct GraphKey {
    int m0, nm, B, mc, T;
    const void *yhat, *ymean, *noise, *y0, *seq;
    bool operator<(const GraphKey& o) const {
        return std::tie(m0, nm, B, mc, T, yhat, ymean, noise, y0, seq) <
               std::tie(o.m0, o.nm, o.B, o.mc, o.T, o.yhat, o.ymean, o.noise, o.y0, o.seq);
    }
};

struct BatchKey {
    unsigned long long cond;          // the conditioner's serial, not its address (addresses are reused after nd_cond_destroy)
    const void *images, *noise, *samples, *prob, *vote, *probs, *yhat;
    int B, mc, T;
    unsigned temp_bits;
    bool profiling;
    bool operator<(const BatchKey& o) const {
        return std::tie(cond, images, noise, samples, prob, vote, probs, yhat, B, mc, T, temp_bits, profiling) <
               std::tie(o.cond, o.images, o.noise, o.samples, o.prob, o.vote, o.probs, o.yhat, o.B, o.mc, o.T, o.temp_bits, o.profiling);
    }
};

struct nd_handle_s {
    nd_config cfg{};
    char* ws = nullptr;
    size_t ws_bytes = 0;
    std::vector<MemberHost> members;
    MemberDev* members_dev = nullptr;      // [K]
    SkinnyDesc* descs_dev = nullptr;       // [L_COUNT][K]
    std::vector<SkinnyDesc> descs_host;    // the same table on the host: the step launches pass their rows by value (SkinnyInline)
    std::vector<MemberDev> members_host;   // ... and the step head / final kernels theirs (MemberInline)
    SkinnyDesc* spk_dev = nullptr;         // [K]   encoder_x.0 as split-K partial sums (MODE 2)
    SplitKEpiDesc* spke_dev = nullptr;     // [K]
    float *alphas = nullptr, *omabs = nullptr;
    float* xpack = nullptr;                // frag16 [maxB][D] image batch shared by all members
    float* tile_ws = nullptr;              // k-slab accumulators of k_cond_gemm's split tail (large-M steps only)
    bool b9 = false;                       // the large-M step blocks run on the bf16 matrix pipe (frag32b3 copies of lin2 / lin3 exist)
    unsigned long long* rng_state = nullptr;   // {seed, batch counter | first image << 32} of the in-library noise (nd_seed)
    unsigned* input_seq = nullptr;             // calls of nd_predict_batch whose inputs have been consumed (device counter behind input_flag)
    unsigned* input_flag = nullptr;            // caller's host-visible word that receives that count (nd_set_input_flag), or null
    unsigned* persist_bar = nullptr;           // barrier block of the one-launch loop (nd_persist.hpp): per-member arrival counters + sticky error word
    int persist_mode = 0;                      // ND_PERSIST: 0 = per-step kernels (hipGraph form), 1 = one launch per p_sample_loop where nd_persist_plan allows
    int persist_skew_ticks = 0;                // ND_PERSIST_SKEW_US: start offset between consecutive members (100 MHz ticks)
    bool persist_last = false;                 // the most recently recorded / enqueued loop took the one-launch form
    float* noise_ws = nullptr;             // [K][T][max_rows][C] draws of the in-library noise (noise_dev == NULL)
    float* logits_ws = nullptr;            // [K][max_batch][C] guiding-prediction logits of nd_predict_batch
    int sched_T = 0;
    std::vector<int> plan_tau;             // sampler plan (nd_set_sampler): the S timesteps tau_0 < .. < tau_{S-1}, baked into kernel arguments; empty: none
    float* plan_coef = nullptr;            // ... and its [S][4] coefficients (cy, cm, ce, cz) in a device buffer of the handle's own (not the workspace)
    int plan_cap = 0;                      // rows that buffer holds
    int NT = 0, S0 = 0;
    bool enc_splitk = false;
    int half = 0;                          // cfg.operand_dtype == ND_DTYPE_F16
    std::map<GraphKey, hipGraphExec_t> graphs;
    std::map<BatchKey, hipGraphExec_t> batch_graphs;   // nd_predict_batch: the whole hot path of a batch
    hipStream_t capture_stream = nullptr;              // only ever used to RECORD batch graphs, never to run anything
    int encoded_B = -1;
    bool profiling = false;
    std::vector<hipEvent_t> probe_events;   // 4 per probed step i: e0 | head(i) | e1 | lin2, lin3 (i) | e2 | head, lin2, lin3 (i+1) | e3
    int probe_steps = 0;
    int probe_nodes = 0;             // event-record nodes in the most recently built graph (nd_profile_probe_nodes)
};

// nd_handle.hip
int nd_check_range(nd_handle_s* h, int m0, int nm);                    // workspace bound, members m0 .. m0+nm-1 exist and are loaded
void nd_drop_graphs(nd_handle_s* h);                                   // after anything a recorded graph has baked in changes
void nd_note_h_layout(nd_handle_s* h, int m0, int nm, bool split);     // MemberHost::h_split of a member range
// nd_conditioner.hip
int nd_guiding_prediction_first(nd_cond c, const float* images, float* logits_out, float* yhat_out, int B, int n_used, void* stream);
unsigned long long nd_cond_serial(nd_cond c);     // changes with every change of the conditioner's state

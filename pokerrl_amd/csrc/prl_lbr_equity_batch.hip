// LBR check-down equities of MANY independent decisions at once (reference: LocalLBRWorker.py:379-512, one decision per call there).
// prl_lbr_checkdown_equity (prl_lbr_kernels.hip) answers one decision: five allocations, two uploads, a class download, four launches and a device
// synchronisation -- and, with more than two cards to come, ONE dependent float32 chain per candidate range (at most twelve waves on the whole device).
// A round of the batched engine asks for up to a thousand such decisions, and they do not depend on each other. Here they stay in HBM and share the
// launches: every request's chains run side by side, one wave each. The per-board arithmetic is the single call's (the device functions of prl_lbr.h and
// prl_lbr_deep.h, unchanged), so every request's result is the single call's, bit for bit.
//   prl_k_lbre_prepare  : one workgroup per request: the request's record (game, counts, possible cards, offset into the equity buffer) and the class
//                         index lists of the FIRST enumerated board (the reference's quirk, see prl_lbr_kernels.hip)
//   prl_k_lbre_board_eq : blockIdx.y = request, x strides over its (range, board) pairs
//   prl_k_lbre_deep_terms / prl_k_lbre_deep_sum : more than two cards to come: a lane per (request, range, prefix), then a wave per (request, range)
//   prl_k_lbre_reduce   : at most two cards to come: a lane per (request, range)
// Requests of a call may differ in the number of cards on the table: they are processed in groups of equal n_dealt (a grid is shaped by the number
// of boards). The equity buffer holds sum(n_q * n_boards) floats -- 102 MB for one pre-flop request of twelve ranges -- so the requests go through it in
// chunks that fit a budget (PRL_LBR_EQ_BATCH_MB, default 8 GiB: about 80 pre-flop requests, ~960 chains).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "prl_device.h"
#include "prl_host.h"
#include "prl_lbr.h"
#include "prl_lbr_deep.h"
#include "prl_lbr_equity_batch.h"
#include "prl_rt.h"

extern "C" int32_t prl_device_available(void);
int prl_hole_lut_device(const uint16_t** out);  // prl_capi_device.hip: device-resident [1326] c1 | c2 << 8

#define LBRE_PC_BYTES 56  // the possible cards of a request (<= 52), padded to words
#define LBRE_PREP_THREADS 256

struct PrlLbrEqPlan {  // what the host decides per request: its place in the processing order is its index
    int32_t req, pad;
    long long eq_off;  // floats into the chunk's equity buffer
};
struct PrlLbrEqRec {  // what the kernels read per request (wave-uniform addresses: it stays in scalar registers)
    PrlLbrGame g;
    int32_t req, n_q, n_boards, n_prefix, n_pc, lbr_idx, n_big, n_eq;
    long long eq_off;
    int8_t pc[LBRE_PC_BYTES];  // the cards that can still come, ascending
};
static_assert(sizeof(PrlLbrEqRec) % 8 == 0 && sizeof(PrlLbrEqRec) <= 144, "the record is copied by words and has a fixed LDS slot");

static size_t lbre_prepare_smem(int R) { return 144 + 2 * LBRE_PREP_THREADS * sizeof(int) + (((size_t)R + 15) & ~(size_t)15); }

PRL_GLOBAL void PRL_LAUNCH_BOUNDS(LBRE_PREP_THREADS) prl_k_lbre_prepare(PrlLbrGame g0, const PrlLbrEqPlan* __restrict__ plan, int p0, const int32_t* __restrict__ meta,
                                                                        PrlLbrEqRec* __restrict__ rec, uint16_t* __restrict__ lists, int lstride) {
    char* sm = prl_smem();
    PrlLbrEqRec* S = (PrlLbrEqRec*)sm;
    int* cnt = (int*)(sm + 144);                                          // [2][threads]: hands of class 1 / 2 in a lane's segment, then their exclusive prefix
    uint8_t* cls = (uint8_t*)(sm + 144 + 2 * LBRE_PREP_THREADS * sizeof(int));  // [R]
    const int tid = (int)prl_tid(), nt = LBRE_PREP_THREADS;
    const int p = p0 + (int)prl_bid();
    if (tid == 0) {
        const PrlLbrEqPlan pl = plan[p];
        const int32_t* m = meta + (size_t)pl.req * 8;
        PrlLbrGame g = g0;
        g.n_dealt = m[2]; g.n_to_deal = g.n_board_total - m[2];
        for (int i = 0; i < 5; ++i) g.board[i] = i < g.n_dealt ? (int8_t)m[3 + i] : (int8_t)0;
        int c1 = m[0], c2 = 0;
        if (g.n_hole == 2) prl_hole_cards_2(m[0], g.n_cards, &c1, &c2);
        g.lbr_hand[0] = (int8_t)c1; g.lbr_hand[1] = (int8_t)c2; g.pad = 0;
        S->g = g;
        S->req = pl.req; S->n_q = m[1]; S->lbr_idx = m[0]; S->eq_off = pl.eq_off;
        for (int i = 0; i < LBRE_PC_BYTES; ++i) S->pc[i] = 0;
        const int n_pc = prl_lbr_possible_cards(g, S->pc);
        S->n_pc = n_pc;
        S->n_boards = (int)prl_comb(n_pc, g.n_to_deal);
        S->n_prefix = g.n_to_deal > 2 ? (int)prl_comb(n_pc - 1, g.n_to_deal - 1) : 0;
        S->n_big = 0; S->n_eq = 0;
    }
    prl_sync();
    const PrlLbrGame g = S->g;
    const int R = g.R, lbr_idx = S->lbr_idx;
    int8_t fb[5];  // the first board of the enumeration: the cards on the table, then the lowest cards that can come
    for (int i = 0; i < 5; ++i) fb[i] = i < g.n_dealt ? g.board[i] : (i < g.n_board_total ? S->pc[i - g.n_dealt] : (int8_t)0);
    // a lane owns a run of consecutive hands, so that "ascending" is "lane by lane"
    const int per = (R + nt - 1) / nt;
    const int h0 = tid * per < R ? tid * per : R, h1 = h0 + per < R ? h0 + per : R;
    int n1 = 0, n2 = 0;
    for (int h = h0; h < h1; ++h) {
        const uint8_t c = prl_lbr_classify_hand(g, lbr_idx, h, fb);
        cls[h] = c;
        n1 += c == 1; n2 += c == 2;
    }
    cnt[tid] = n1; cnt[nt + tid] = n2;
    prl_sync();
    if (tid == 0) {  // exclusive prefix over the lanes' counts (256 entries, once per request)
        int a = 0, b = 0;
        for (int i = 0; i < nt; ++i) {
            const int x = cnt[i], y = cnt[nt + i];
            cnt[i] = a; cnt[nt + i] = b;
            a += x; b += y;
        }
        S->n_big = a; S->n_eq = b;
    }
    prl_sync();
    // the hands LBR beats in ascending order, then the ties in ascending order, zero-padded (the class streams fetch eight entries at a time)
    uint16_t* L = lists + (size_t)p * lstride;
    const int n_big = S->n_big, n_eq = S->n_eq;
    int o1 = cnt[tid], o2 = n_big + cnt[nt + tid];
    for (int h = h0; h < h1; ++h) {
        const uint8_t c = cls[h];
        if (c == 1) L[o1++] = (uint16_t)h;
        else if (c == 2) L[o2++] = (uint16_t)h;
    }
    for (int i = n_big + n_eq + tid; i < lstride; i += nt) L[i] = 0;
    int32_t* dst = (int32_t*)(rec + p);
    const int32_t* src = (const int32_t*)S;
    for (int i = tid; i < (int)(sizeof(PrlLbrEqRec) / 4); i += nt) dst[i] = src[i];
}

// the request's possible cards into LDS: the board of a pair is un-ranked with per-lane indices into them, which an array in registers cannot serve
PRL_DEV PRL_INLINE void lbre_load_pc(const PrlLbrEqRec& r, int8_t* pc) {
    const int tid = (int)prl_tid();
    if (tid < LBRE_PC_BYTES) pc[tid] = r.pc[tid];
    prl_sync();
}

PRL_GLOBAL void PRL_LAUNCH_BOUNDS(64) prl_k_lbre_board_eq(const PrlLbrEqRec* __restrict__ rec, int p0, const uint16_t* __restrict__ lists, int lstride,
                                                          const float* __restrict__ ranges, long long r_stride, float* __restrict__ eq, const uint16_t* __restrict__ hole_lut) {
    const int p = p0 + (int)prl_bid_y();
    const PrlLbrEqRec& r = rec[p];
    int8_t* pc = (int8_t*)prl_smem();
    lbre_load_pc(r, pc);
    const PrlLbrGame g = r.g;
    const int n_boards = r.n_boards, n_pc = r.n_pc, n_big = r.n_big, n_eq = r.n_eq;
    const uint16_t* L = lists + (size_t)p * lstride;
    const float* rg = ranges + (size_t)r.req * r_stride;
    float* e = eq + r.eq_off;
    const long long total = (long long)r.n_q * n_boards;
    for (long long t = (long long)prl_bid() * prl_nthreads() + prl_tid(); t < total; t += (long long)prl_nblocks() * prl_nthreads()) {
        const int q = (int)(t / n_boards), b = (int)(t - (long long)q * n_boards);
        int8_t fb[5];
        prl_lbr_board_unrank(g, pc, n_pc, b, fb);
        e[t] = prl_lbr_board_equity_lists(g, fb, L, n_big, n_eq, rg + (size_t)q * g.R, hole_lut);
    }
}

// LDS: [n_cards][256] card probabilities (prl_lbr_deep_terms_lane), then the possible cards
PRL_GLOBAL void PRL_LAUNCH_BOUNDS(256) prl_k_lbre_deep_terms(const PrlLbrEqRec* __restrict__ rec, int p0, const float* __restrict__ ranges, long long r_stride, float* __restrict__ eq) {
    const PrlLbrEqRec& r = rec[p0 + (int)prl_bid_y()];
    const int nt = (int)prl_nthreads(), tid = (int)prl_tid();
    float* cp_all = (float*)prl_smem();
    int8_t* pc = (int8_t*)(cp_all + (size_t)r.g.n_cards * nt);
    lbre_load_pc(r, pc);
    const long long t = (long long)prl_bid() * nt + tid;
    if (t >= (long long)r.n_q * r.n_prefix) return;
    const int q = (int)(t / r.n_prefix);
    const int pr = (int)(t - (long long)q * r.n_prefix);
    const PrlLbrGame g = r.g;
    prl_lbr_deep_terms_lane(g, pc, r.n_pc, ranges + (size_t)r.req * r_stride + (size_t)q * g.R, pr, cp_all, nt, tid, eq + r.eq_off + (size_t)q * r.n_boards);
}

// one wave per (request, range): x = range, y = request; every chain of a chunk in one launch
PRL_GLOBAL void PRL_LAUNCH_BOUNDS(64) prl_k_lbre_deep_sum(const PrlLbrEqRec* __restrict__ rec, int p0, const float* __restrict__ eq, float* __restrict__ wp, int q_stride) {
    const PrlLbrEqRec& r = rec[p0 + (int)prl_bid_y()];
    const int q = (int)prl_bid(), lane = (int)prl_tid();
    if (q >= r.n_q) return;
    const float s = prl_lbr_deep_sum_wave(r.g.n_to_deal, r.n_boards, eq + r.eq_off + (size_t)q * r.n_boards, lane);
    if (lane == 0) wp[(size_t)r.req * q_stride + q] = s;
}

PRL_GLOBAL void PRL_LAUNCH_BOUNDS(64) prl_k_lbre_reduce(const PrlLbrEqRec* __restrict__ rec, int p0, int n, const float* __restrict__ ranges, long long r_stride,
                                                        const float* __restrict__ eq, float* __restrict__ wp, int q_stride) {
    const int total = n * q_stride;
    for (int t = (int)(prl_bid() * prl_nthreads() + prl_tid()); t < total; t += (int)(prl_nblocks() * prl_nthreads())) {
        const PrlLbrEqRec& r = rec[p0 + t / q_stride];
        const int q = t % q_stride;
        if (q >= r.n_q) continue;
        const PrlLbrGame g = r.g;
        wp[(size_t)r.req * q_stride + q] = prl_lbr_reduce_range(g, ranges + (size_t)r.req * r_stride + (size_t)q * g.R, eq + r.eq_off + (size_t)q * r.n_boards);
    }
}

void prl_lbr_eq_work_free(PrlLbrEqWork* w) {
    (void)hipFree(w->plan); (void)hipFree(w->rec); (void)hipFree(w->lists); (void)hipFree(w->eq);
    *w = PrlLbrEqWork();
}

template <class T>
static bool lbre_grow(T** p, size_t* cap, size_t need, size_t elem_bytes) {
    if (need <= *cap) return true;
    (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    if (hipMalloc((void**)p, need * elem_bytes) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return false; }
    *cap = need;
    return true;
}

static bool lbre_game(const PrlRules* rules, PrlLbrGame* g) {
    memset(g, 0, sizeof(*g));
    g->n_hole = rules->n_hole_cards; g->n_cards = rules->n_cards; g->n_suits = rules->n_suits; g->rank_rule = rules->rank_rule; g->R = rules->range_size;
    g->n_board_total = rules->n_board_cards;
    return !(g->n_hole < 1 || g->n_hole > 2 || g->n_cards > PRL_LBR_MAX_CARDS || g->n_board_total > 5 || (g->n_hole == 2 && (g->n_cards != 52 || g->n_board_total != 5)));
}

int prl_lbr_equity_batch_device(const PrlRules* rules, int n_req, const int32_t* h_meta, const int32_t* d_meta, const float* d_ranges, int q_stride,
                                float* d_wp, void* stream, PrlLbrEqWork* work, int* out_chunks) {
    if (out_chunks) *out_chunks = 0;
    if (!rules || !h_meta || !d_meta || !d_ranges || !d_wp || !work || n_req <= 0 || q_stride <= 0) { prl_set_error("bad argument"); return PRL_ERR_ARG; }
    PrlLbrGame g0;
    if (!lbre_game(rules, &g0)) { prl_set_error("LBR: 1-hole-card games or 52-card hold'em with 5 board cards"); return PRL_ERR_UNSUPPORTED; }
    if (g0.n_board_total > PRL_LBR_MAX_DEAL) { prl_set_error("LBR equity: at most 5 board cards to come"); return PRL_ERR_UNSUPPORTED; }
    const int R = g0.R;
    // every request checked here, on the host copy: the kernels index with these numbers
    struct Item { int req, n_dealt, k, n_q, n_boards, n_prefix; long long need; };
    std::vector<Item> items((size_t)n_req);
    long long largest = 0;
    for (int i = 0; i < n_req; ++i) {
        const int32_t* m = h_meta + (size_t)i * 8;
        bool ok = m[0] >= 0 && m[0] < R && m[1] >= 1 && m[1] <= q_stride && m[2] >= 0 && m[2] <= g0.n_board_total;
        for (int j = 0; ok && j < m[2]; ++j) ok = m[3 + j] >= 0 && m[3 + j] < g0.n_cards;
        if (!ok) { prl_set_error("LBR equity batch: a request is out of range (hand index, n_q, n_dealt or a table card)"); return PRL_ERR_ARG; }
        Item& it = items[(size_t)i];
        it.req = i; it.n_dealt = m[2]; it.k = g0.n_board_total - m[2]; it.n_q = m[1];
        const int n_pc = g0.n_cards - g0.n_hole - m[2];
        const long long nb = prl_comb(n_pc, it.k);
        if (nb <= 0 || it.n_q * nb > 0x7FFFFFFFll) { prl_set_error("LBR equity: too many (range, board) pairs in one request"); return PRL_ERR_ARG; }
        it.n_boards = (int)nb;
        it.n_prefix = it.k > 2 ? (int)prl_comb(n_pc - 1, it.k - 1) : 0;
        it.need = it.n_q * nb;
        largest = std::max(largest, it.need);
    }
    // fewest cards on the table first: the requests with running-sum chains lead every chunk, groups of equal n_dealt are neighbours
    std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.n_dealt < b.n_dealt; });
    long long budget = 8192ll << 18;  // floats
    if (const char* ev = getenv("PRL_LBR_EQ_BATCH_MB")) { const long long mb = atoll(ev); if (mb > 0) budget = mb << 18; }
    const int max_chunk_req = 32768;  // blockIdx.y counts a chunk's requests
    std::vector<int> chunk_begin;
    std::vector<PrlLbrEqPlan> plan((size_t)n_req);
    for (;;) {  // a budget the device cannot give is halved, down to the largest single request
        chunk_begin.clear();
        long long used = 0, chunk_max = 0;
        for (int i = 0; i < n_req; ++i) {
            const bool open_new = chunk_begin.empty() || used + items[(size_t)i].need > budget || i - chunk_begin.back() >= max_chunk_req;
            if (open_new) { chunk_begin.push_back(i); used = 0; }
            plan[(size_t)i].req = items[(size_t)i].req; plan[(size_t)i].pad = 0; plan[(size_t)i].eq_off = used;
            used += items[(size_t)i].need;
            chunk_max = std::max(chunk_max, used);
        }
        if (lbre_grow(&work->eq, &work->cap_eq, (size_t)chunk_max, sizeof(float))) break;
        if (budget <= largest) { prl_set_error("LBR equity batch: hipMalloc of the equity buffer failed"); return PRL_ERR_HIP; }
        budget = std::max(largest, std::min(budget, chunk_max) / 2);
    }
    chunk_begin.push_back(n_req);
    const int lstride = (R + 8 + 7) & ~7;
    if (!lbre_grow((PrlLbrEqPlan**)&work->plan, &work->cap_plan, (size_t)n_req, sizeof(PrlLbrEqPlan)) ||
        !lbre_grow((PrlLbrEqRec**)&work->rec, &work->cap_rec, (size_t)n_req, sizeof(PrlLbrEqRec)) ||
        !lbre_grow(&work->lists, &work->cap_lists, (size_t)n_req * lstride, sizeof(uint16_t))) {
        prl_set_error("LBR equity batch: hipMalloc failed"); return PRL_ERR_HIP;
    }
    const uint16_t* hole_lut = nullptr;  // hold'em: the process-wide (c1, c2) table of the hand evaluator
    if (g0.n_hole == 2 && prl_hole_lut_device(&hole_lut) != PRL_OK) return PRL_ERR_HIP;
    const PrlLbrEqPlan* d_plan = (const PrlLbrEqPlan*)work->plan;
    PrlLbrEqRec* d_rec = (PrlLbrEqRec*)work->rec;
    PRL_HIP_TRY(hipMemcpy(work->plan, plan.data(), (size_t)n_req * sizeof(PrlLbrEqPlan), hipMemcpyHostToDevice));
    const long long r_stride = (long long)q_stride * R;
    for (size_t c = 0; c + 1 < chunk_begin.size(); ++c) {
        const int begin = chunk_begin[c], end = chunk_begin[c + 1];
        PRL_LAUNCH(prl_k_lbre_prepare, end - begin, LBRE_PREP_THREADS, lbre_prepare_smem(R), stream, g0, d_plan, begin, d_meta, d_rec, work->lists, lstride);
        int deep_end = begin, q_max_deep = 0;
        for (int a = begin; a < end;) {  // the groups of equal n_dealt
            int b = a;
            long long pairs_max = 0, prefixes_max = 0;
            for (; b < end && items[(size_t)b].n_dealt == items[(size_t)a].n_dealt; ++b) {
                pairs_max = std::max(pairs_max, items[(size_t)b].need);
                prefixes_max = std::max(prefixes_max, (long long)items[(size_t)b].n_q * items[(size_t)b].n_prefix);
                if (items[(size_t)b].k > 2) q_max_deep = std::max(q_max_deep, items[(size_t)b].n_q);
            }
            const int n = b - a;
            const long long gx_cap = std::max(1ll, 262144ll / n);
            const int gx = (int)std::min((pairs_max + 63) / 64, gx_cap);
            PRL_LAUNCH_XY(prl_k_lbre_board_eq, gx, n, 64, 64, stream, (const PrlLbrEqRec*)d_rec, a, (const uint16_t*)work->lists, lstride, d_ranges, r_stride, work->eq, hole_lut);
            if (items[(size_t)a].k > 2) {
                PRL_LAUNCH_XY(prl_k_lbre_deep_terms, (int)((prefixes_max + 255) / 256), n, 256, (size_t)g0.n_cards * 256 * sizeof(float) + 64, stream, (const PrlLbrEqRec*)d_rec, a,
                              d_ranges, r_stride, work->eq);
                deep_end = b;
            }
            a = b;
        }
        if (deep_end > begin)
            PRL_LAUNCH_XY(prl_k_lbre_deep_sum, q_max_deep, deep_end - begin, 64, 0, stream, (const PrlLbrEqRec*)d_rec, begin, (const float*)work->eq, d_wp, q_stride);
        if (end > deep_end) {
            const int n = end - deep_end;
            PRL_LAUNCH(prl_k_lbre_reduce, ((long long)n * q_stride + 63) / 64, 64, 0, stream, (const PrlLbrEqRec*)d_rec, deep_end, n, d_ranges, r_stride, (const float*)work->eq,
                       d_wp, q_stride);
        }
    }
    PRL_HIP_TRY(hipGetLastError());
    PRL_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (out_chunks) *out_chunks = (int)chunk_begin.size() - 1;
    return PRL_OK;
}

extern "C" int32_t prl_lbr_checkdown_equity_batch(const PrlRules* rules, int32_t n_req, const int8_t* boards_dealt, const int32_t* n_dealt, const int8_t* lbr_hands,
                                                  const float* ranges, const int32_t* n_q, int32_t q_stride, float* out_wp) {
    if (!rules || !n_dealt || !lbr_hands || !ranges || !n_q || !out_wp || n_req <= 0 || q_stride <= 0) { prl_set_error("bad argument"); return PRL_ERR_ARG; }
    for (int i = 0; i < n_req; ++i)
        if (n_q[i] <= 0 || n_q[i] > q_stride || n_dealt[i] < 0 || (n_dealt[i] > 0 && !boards_dealt)) { prl_set_error("bad argument"); return PRL_ERR_ARG; }
    if (!prl_device_available()) { prl_set_error("no HIP device: LBR has no CPU fallback"); return PRL_ERR_NO_DEVICE; }
    PrlLbrGame g0;
    if (!lbre_game(rules, &g0)) { prl_set_error("LBR: 1-hole-card games or 52-card hold'em with 5 board cards"); return PRL_ERR_UNSUPPORTED; }
    const int nh = g0.n_hole, R = g0.R;
    std::vector<int32_t> meta((size_t)n_req * 8);
    for (int i = 0; i < n_req; ++i) {
        if (g0.n_board_total - n_dealt[i] < 0 || g0.n_board_total - n_dealt[i] > PRL_LBR_MAX_DEAL) { prl_set_error("LBR equity: at most 5 board cards to come"); return PRL_ERR_UNSUPPORTED; }
        int32_t* m = &meta[(size_t)i * 8];
        int c1 = lbr_hands[(size_t)i * nh], c2 = nh == 2 ? lbr_hands[(size_t)i * nh + 1] : 0;
        if (nh == 2 && c1 > c2) std::swap(c1, c2);  // (an unsorted hand: as the single call)
        if (c1 < 0 || c1 >= g0.n_cards || (nh == 2 && (c2 >= g0.n_cards || c1 == c2))) { prl_set_error("LBR equity batch: a hand's cards are out of range"); return PRL_ERR_ARG; }
        m[0] = nh == 1 ? c1 : prl_range_idx_2(c1, c2, g0.n_cards);
        m[1] = n_q[i]; m[2] = n_dealt[i];
        for (int j = 0; j < 5; ++j) m[3 + j] = j < n_dealt[i] ? (int32_t)boards_dealt[(size_t)i * 5 + j] : -1;
    }
    int32_t* d_meta = nullptr; float *d_rg = nullptr, *d_wp = nullptr;
    PrlLbrEqWork work;
    const size_t n_rg = (size_t)n_req * q_stride * R, n_wp = (size_t)n_req * q_stride;
    int rc = PRL_OK;
#define LE_TRY(x) do { if ((x) != hipSuccess) { (void)hipGetLastError(); prl_set_error("HIP error in prl_lbr_checkdown_equity_batch"); rc = PRL_ERR_HIP; goto done; } } while (0)
    LE_TRY(hipMalloc((void**)&d_meta, meta.size() * sizeof(int32_t)));
    LE_TRY(hipMalloc((void**)&d_rg, n_rg * sizeof(float)));
    LE_TRY(hipMalloc((void**)&d_wp, n_wp * sizeof(float)));
    LE_TRY(hipMemcpy(d_meta, meta.data(), meta.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    LE_TRY(hipMemcpy(d_rg, ranges, n_rg * sizeof(float), hipMemcpyHostToDevice));
    LE_TRY(hipMemcpy(d_wp, out_wp, n_wp * sizeof(float), hipMemcpyHostToDevice));  // slots at or beyond n_q keep what the caller put there
    rc = prl_lbr_equity_batch_device(rules, n_req, meta.data(), d_meta, d_rg, q_stride, d_wp, nullptr, &work, nullptr);
    if (rc != PRL_OK) goto done;
    LE_TRY(hipMemcpy(out_wp, d_wp, n_wp * sizeof(float), hipMemcpyDeviceToHost));
#undef LE_TRY
done:
    (void)hipFree(d_meta); (void)hipFree(d_rg); (void)hipFree(d_wp);
    prl_lbr_eq_work_free(&work);
    return rc;
}

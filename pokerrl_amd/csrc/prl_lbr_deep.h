// Device pieces of the LBR check-down equity that more than one kernel file runs: the stand-alone call (prl_lbr_kernels.hip, one decision) and
// the batched core (prl_lbr_equity_batch.hip, a round's decisions side by side). One copy of each, so that both issue the same float32 operations
// in the same order.
#pragma once
#include "prl_device.h"
#include "prl_lbr.h"

// the b-th board of the enumeration, any number of cards to come: the lexicographic k-combination number b of the possible cards (what the host
// used to enumerate and upload: 10.6 MB per pre-flop call)
PRL_HD PRL_INLINE void prl_lbr_board_unrank(const PrlLbrGame& g, const int8_t* pc, int n_pc, long long b, int8_t* fb) {
    const int k = g.n_to_deal;
    for (int i = 0; i < 5; ++i) fb[i] = i < g.n_dealt ? g.board[i] : (int8_t)0;
    int v = 0;
    for (int j = 0; j < k; ++j) {
        for (;; ++v) {
            const long long below = prl_comb(n_pc - 1 - v, k - 1 - j);  // boards that continue with card v at position j
            if (b < below) break;
            b -= below;
        }
        const int8_t c = pc[v++];
        for (int i = 0; i < 5; ++i) fb[i] = i == g.n_dealt + j ? c : fb[i];  // (selects: a write at a run-time position would push the board into private memory)
    }
}

// One lane of the deal tree's terms (more than two cards to come): prefix number `pr` of the first k - 1 cards to come of range rg. The chain of
// re-normalised card probabilities down ITS path (the same operations on the same numbers as prl_lbr_reduce_range_deep's walk), then
// x[b] = e[b] * reach for the boards below the prefix -- they are consecutive in the enumeration order -- written over e[b].
// cp_all: [n_cards][nt] work floats in LDS, lane index fastest (no bank conflicts); e: the range's n_boards equities.
PRL_DEV PRL_INLINE void prl_lbr_deep_terms_lane(const PrlLbrGame& g, const int8_t* pc, int n_pc, const float* rg, int pr, float* cp_all, int nt, int tid, float* e_range) {
    const int k = g.n_to_deal, nc = g.n_cards;
    auto cp = [&](int c) -> float& { return cp_all[(size_t)c * nt + tid]; };
    // the prefix: combination number `pr` of k - 1 of the first n_pc - 1 possible cards, lexicographic (the walk's order of interior paths)
    int idx[PRL_LBR_MAX_DEAL];
    {
        int v = 0;
        for (int j = 0; j < k - 1; ++j) {
            for (;; ++v) {
                const int below = (int)prl_comb(n_pc - 1 - (v + 1), k - 2 - j);  // prefixes that continue with card v at position j
                if (pr < below) break;
                pr -= below;
            }
            idx[j] = v++;
        }
    }
    // rank of the first board below the prefix among all boards (lexicographic k-combinations of n_pc cards)
    long long b0 = 0;
    {
        int prev = -1;
        for (int j = 0; j < k - 1; ++j) {
            for (int v = prev + 1; v < idx[j]; ++v) b0 += prl_comb(n_pc - 1 - v, k - 1 - j);
            prev = idx[j];
        }
    }
    // the chain of card probabilities down the path (prl_lbr_reduce_range_deep, level by level; one array, rewritten in place)
    for (int c = 0; c < nc; ++c) cp(c) = prl_lbr_card_not_held(g, rg, c);
    for (int i = 0; i < g.n_hole; ++i) cp(g.lbr_hand[i]) = 0.f;
    for (int i = 0; i < g.n_dealt; ++i) cp(g.board[i]) = 0.f;
    {
        int j = 0;
        auto nx = [&]() { return cp(j++); };
        const float s = prl_np_sum_stream<0>(nc, nx);
        if (s > 0.f)
            for (int c = 0; c < nc; ++c) cp(c) = cp(c) / s;
    }
    float reach = 1.f;
    for (int l = 0; l < k - 1; ++l) {
        const int card = pc[idx[l]];
        reach = l == 0 ? cp(card) : reach * cp(card);  // 1.0 * p at depth 0
        cp(card) = 0.f;
        int j = 0;
        auto nx = [&]() { return cp(j++); };
        const float s = prl_np_sum_stream<0>(nc, nx);
        for (int c = 0; c < nc; ++c) cp(c) = cp(c) / s;
    }
    float* e = e_range + b0;
    int b = 0;
    for (int i = idx[k - 2] + 1; i < n_pc; ++i, ++b) {
        const float r = k == 1 ? cp(pc[i]) : reach * cp(pc[i]);
        e[b] = e[b] * r;
    }
}

// The running float32 sum of a range's terms in board order, by one WAVE. The sum is a strictly sequential float32 chain (that is the reference's
// order); what can be taken off the chain is everything but the add itself: the wave loads 64 terms per register (coalesced, eight registers in
// flight), and every lane runs the same chain taking term j of a register by a lane broadcast (v_readlane: a scalar operand, independent of the
// chain) -- the chain is one dependent v_add per term. Every lane returns the sum times k! (LocalLBRWorker.py:463-468).
#if defined(PRL_EMU)
#define PRL_LANE_BCAST(v, j) prl_shfl((v), (j))
#define PRL_SCHED_FENCE() do { } while (0)
#else
#define PRL_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
PRL_DEV PRL_INLINE float prl_lane_bcast_(float v, int j) { int i; __builtin_memcpy(&i, &v, 4); i = __builtin_amdgcn_readlane(i, j); float o; __builtin_memcpy(&o, &i, 4); return o; }
#define PRL_LANE_BCAST(v, j) prl_lane_bcast_((v), (j))
#endif
PRL_DEV PRL_INLINE float prl_lbr_deep_sum_wave(int k, int n_boards, const float* __restrict__ x, int lane) {
    float win = 0.f;
    bool first = true;
    for (int b0 = 0; b0 < n_boards; b0 += 8 * 64) {
        float v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) { const int i = b0 + r * 64 + lane; v[r] = i < n_boards ? x[i] : 0.f; }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int left = n_boards - (b0 + r * 64);
            if (left >= 64 && !first) {
                // sixteen broadcasts, a scheduling fence, sixteen adds: left to itself the compiler reads every lane into ONE scalar register right before
                // its add (v_readlane, s_nop 1, v_add: 19 clocks per term); sixteen live scalars take the broadcasts off the chain
#pragma unroll
                for (int j0 = 0; j0 < 64; j0 += 16) {
                    float t[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j) t[j] = PRL_LANE_BCAST(v[r], j0 + j);
                    PRL_SCHED_FENCE();
#pragma unroll
                    for (int j = 0; j < 16; ++j) win = win + t[j];
                    PRL_SCHED_FENCE();
                }
            } else {
                for (int j = 0; j < 64; ++j) {
                    const float t = PRL_LANE_BCAST(v[r], j);
                    if (j < left) { win = first ? t : win + t; first = false; }  // 0.0 (Python float) + float32 -> float32
                }
            }
        }
    }
    float fact = 1.f;
    for (int m = 2; m <= k; ++m) fact = fact * (float)m;
    return win * fact;
}

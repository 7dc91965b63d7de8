// The heads-up "simple" env observation (PokerEnv.py:199-261, :989-1031, :1253-1271), ONE definition for every producer of observation vectors:
// the batched env (prl_envbatch.hip: the observation of every step) and the public-tree observations (prl_tree_obs.hip: what a neural agent
// sees at a tree node). Host + device.
#pragma once
#include "prl_defs.h"
#include "prl_env.h"

struct EbFull {
    PrlRules rules;
    int32_t n_deal, obs_dim, suits_matter;
    double reward_scalar;
};
PRL_HD PRL_INLINE int eb_obs_dim(const PrlRules& r) { return 7 + 3 + 2 + 2 + r.n_rounds + 3 * 2 + r.n_board_cards * (r.n_ranks + r.n_suits); }
PRL_HD PRL_INLINE int eb_cards_out(const PrlRules& r, int round) {  // board cards on the table in `round`
    int n = 0;
    for (int k = 1; k <= round && k < 4; ++k) n += r.board_cards_in_round[k];
    return n;
}
// board card i (a constant after unrolling) of a 1- or 2-hole-card game
#define EB_BOARD(c, n_hole, i) ((n_hole) == 2 ? (c)[4 + (i)] : (c)[2 + (i)])
// the heads-up "simple" observation (PokerEnv.py:199-261, :989-1031, :1253-1271): float64 quotients rounded to float32 like the
// reference's np.array(list of Python floats, dtype=float32)
PRL_HD PRL_INLINE void eb_observation(const PrlGame& g, const EbFull& F, const PrlEnvState& s, const int8_t* cards, float* o, size_t stride) {
    const double norm = (double)(g.start_stack[0] + g.start_stack[1]) / 2.0;
    const int small = s.bet[0] < s.bet[1] ? s.bet[0] : s.bet[1], big = s.bet[0] < s.bet[1] ? s.bet[1] : s.bet[0];
    const int min_raise = big + ((big - small) > g.big_blind ? (big - small) : g.big_blind);
    const bool have_la = s.last_action[0] >= 0;
    int k = 0;
    auto put = [&](double v) { o[(size_t)k * stride] = (float)v; ++k; };
    put((double)g.ante / norm); put((double)g.small_blind / norm); put((double)g.big_blind / norm); put((double)min_raise / norm);
    put((double)s.main_pot / norm); put((double)big / norm); put(have_la ? (double)s.last_action[1] / norm : 0.0);
    for (int a = 0; a < 3; ++a) put(have_la && s.last_action[0] == a ? 1.0 : 0.0);
    for (int p = 0; p < 2; ++p) put(have_la && s.last_action[2] == p ? 1.0 : 0.0);
    for (int p = 0; p < 2; ++p) put(s.cur == p ? 1.0 : 0.0);
    for (int r = 0; r < F.rules.n_rounds; ++r) put(s.round == r ? 1.0 : 0.0);
    for (int p = 0; p < 2; ++p) { put((double)s.stack[p] / norm); put((double)s.bet[p] / norm); put(s.allin[p] ? 1.0 : 0.0); }
    const int n_out = eb_cards_out(F.rules, s.round);
    const int8_t* board = cards + 2 * F.rules.n_hole_cards;
    for (int i = 0; i < F.rules.n_board_cards; ++i) {
        const int c = i < n_out ? board[i] : -1;
        const int rank = c >= 0 ? c / F.rules.n_suits : -1, suit = c >= 0 ? c % F.rules.n_suits : -1;
        for (int j = 0; j < F.rules.n_ranks; ++j) put(j == rank ? 1.0 : 0.0);
        for (int j = 0; j < F.rules.n_suits; ++j) put(F.suits_matter && j == suit ? 1.0 : 0.0);
    }
}
// ---- the observation vectors of a workgroup's envs, written as ONE linear stream (round 4) -------------------------------------------------------
// A lane that writes its own env's vector stores 4 bytes at a stride of obs_dim floats: every store instruction of a wave touches 64 cache lines and
// the 436-byte vector of a hold'em env costs 109 of them. Every element of the vector is a function of ONE small word of the env, though: a float
// copied (seven pot / bet quotients, two stacks, two bets) or 1.0 where an integer (last action, who acted, whose turn, round, all-in flag, a
// board card's rank / suit) equals the element's own value. So each lane leaves its env's <= 27 SOURCE WORDS in an LDS row, and the workgroup then
// writes the vectors of its 256 consecutive envs -- one contiguous piece of memory -- with linear, fully coalesced stores: element m of the piece
// belongs to env m / obs_dim, entry m % obs_dim, whose table entry says which word and which comparison.
#define EB_OBS_ROW 29  // words per LDS row (odd: the lanes' row writes hit 64 different banks); [27] = 1: leave this env's vector alone
#define EB_OBS_SKIP 27
PRL_HD PRL_INLINE size_t eb_obs_tab_bytes(int obs_dim) { return (((size_t)obs_dim * 4 + 15) & ~(size_t)15) + 16; }  // the entry table + eb_obs_const(0..2)
PRL_HD PRL_INLINE size_t eb_obs_smem(int obs_dim, int n_threads) { return eb_obs_tab_bytes(obs_dim) + (size_t)n_threads * EB_OBS_ROW * 4; }
// table entry of element j: source word | (value + 1) << 8, value + 1 == 0 for a float that is copied. Source words: 0..6 the seven quotients of
// eb_observation's first line, 7 last action, 8 who did it, 9 whose turn, 10 round, 11 + 3 p: stack, bet, all-in flag of seat p, 17 + 2 i: rank and
// suit of board card i (-1: not dealt yet / suits do not matter)
PRL_HD PRL_INLINE int32_t eb_obs_entry(const EbFull& F, int j) {
    if (j < 7) return j;
    j -= 7;
    if (j < 3) return 7 | ((j + 1) << 8);
    j -= 3;
    if (j < 2) return 8 | ((j + 1) << 8);
    j -= 2;
    if (j < 2) return 9 | ((j + 1) << 8);
    j -= 2;
    if (j < F.rules.n_rounds) return 10 | ((j + 1) << 8);
    j -= F.rules.n_rounds;
    if (j < 6) { const int p = j / 3, q = j % 3; return q < 2 ? 11 + 3 * p + q : ((13 + 3 * p) | (2 << 8)); }
    j -= 6;
    const int per = F.rules.n_ranks + F.rules.n_suits, i = j / per, q = j % per;
    return q < F.rules.n_ranks ? ((17 + 2 * i) | ((q + 1) << 8)) : ((18 + 2 * i) | ((q - F.rules.n_ranks + 1) << 8));
}
PRL_HD PRL_INLINE uint32_t eb_f32_bits(double v) { const float f = (float)v; uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
// the three quotients every vector starts with (ante, blinds): the game's, not the env's -- three lanes compute them once per workgroup
// (eb_obs_setup), every lane copies them (round 6; they were three float64 divisions per env and step)
PRL_HD PRL_INLINE uint32_t eb_obs_const(const PrlGame& g, int k) {
    const double norm = (double)(g.start_stack[0] + g.start_stack[1]) / 2.0;
    return eb_f32_bits((double)(k == 0 ? g.ante : (k == 1 ? g.small_blind : g.big_blind)) / norm);
}
// the source words of one env (live = false: a finished episode, the reference's all-zero observation); k3: eb_obs_const(0..2)
PRL_HD PRL_INLINE void eb_obs_words(const PrlGame& g, const EbFull& F, const PrlEnvState& s, const int8_t (&c)[16], bool live, const uint32_t* k3, uint32_t* w) {
    w[EB_OBS_SKIP] = 0u;
    if (!live) {
        for (int k = 0; k < 7; ++k) w[k] = 0u;
        for (int k = 7; k < 27; ++k) w[k] = 0xFFFFFFFFu;
        for (int p = 0; p < 2; ++p) { w[11 + 3 * p] = 0u; w[12 + 3 * p] = 0u; }
        return;
    }
    const double norm = (double)(g.start_stack[0] + g.start_stack[1]) / 2.0;
    const int small = s.bet[0] < s.bet[1] ? s.bet[0] : s.bet[1], big = s.bet[0] < s.bet[1] ? s.bet[1] : s.bet[0];
    const int min_raise = big + ((big - small) > g.big_blind ? (big - small) : g.big_blind);
    const bool have_la = s.last_action[0] >= 0;
    const uint32_t q_bet0 = eb_f32_bits((double)s.bet[0] / norm), q_bet1 = eb_f32_bits((double)s.bet[1] / norm);
    w[0] = k3[0]; w[1] = k3[1]; w[2] = k3[2];
    w[3] = eb_f32_bits((double)min_raise / norm); w[4] = eb_f32_bits((double)s.main_pot / norm);
    w[5] = s.bet[0] < s.bet[1] ? q_bet1 : q_bet0;  // big / norm: the larger bet's quotient
    w[6] = have_la ? eb_f32_bits((double)s.last_action[1] / norm) : 0u;
    w[7] = have_la ? (uint32_t)s.last_action[0] : 0xFFFFFFFFu;
    w[8] = have_la ? (uint32_t)s.last_action[2] : 0xFFFFFFFFu;
    w[9] = (uint32_t)s.cur;
    w[10] = (uint32_t)s.round;
    w[11] = eb_f32_bits((double)s.stack[0] / norm); w[12] = q_bet0; w[13] = s.allin[0] ? 1u : 0u;
    w[14] = eb_f32_bits((double)s.stack[1] / norm); w[15] = q_bet1; w[16] = s.allin[1] ? 1u : 0u;
    const int n_out = eb_cards_out(F.rules, s.round);
    for (int i = 0; i < 5; ++i) {
        const int cb = EB_BOARD(c, F.rules.n_hole_cards, i);
        const int cc = (i < F.rules.n_board_cards && i < n_out) ? cb : -1;
        w[17 + 2 * i] = cc >= 0 ? (uint32_t)(cc / F.rules.n_suits) : 0xFFFFFFFFu;
        w[18 + 2 * i] = (cc >= 0 && F.suits_matter) ? (uint32_t)(cc % F.rules.n_suits) : 0xFFFFFFFFu;
    }
}

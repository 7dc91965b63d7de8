// Public-tree node observations on the GPU: what a neural agent is fed at a decision node of the tree, for many nodes at once.
//
// Reference semantics: `wrapper.set_to_public_tree_node_state(node); wrapper.get_current_obs()` (RecurrentHistoryWrapper.py:57-85,
// FlatHULimitPokerHistoryWrapper.py:93-114, Vanilla.py), the host walk of this package being pokerrl_amd/game/wrappers.py:history_of_nodes.
//   * env states: the state of a node is prl_env_step(state of its parent, its action) -- the tree builder's own step (prl_tree.cpp);
//     a chance outcome (action -1 below a chance node) takes its chance parent's post-step state and its cards from its board_id row
//     (PublicTree._env_state_of). One launch per tree level; the states stay in HBM with the tree (n_nodes x sizeof(PrlEnvState)).
//     The cache holds the state AFTER every node's action: for chance and terminal nodes that is not PublicTree's "before the money
//     moves" state, but no observation reads those nodes.
//   * rows: a requested node's history is the observation of every decision node on its root path (chance nodes skipped, as in
//     wrappers._path_to_root), root first or inverted. Vanilla writes one row, Flat one row plus the one-hot action-history vector built
//     along the path as FlatHULimitPokerHistoryWrapper._pushback does (offsets from the Python builder).
//   * the observation itself is the env batch's (prl_obs.h: eb_obs_entry / eb_obs_words), and so are the stores: every lane of a
//     workgroup leaves one row's source words in LDS, then consecutive lanes write consecutive floats of the rows (each row lands at its
//     own destination; rows that follow each other in memory make one linear stream).
//   * legal-action masks [n][n_actions] from first_col / n_children / col_action.
#include <string.h>

#include <string>
#include <vector>

#include "prl_device.h"
#include "prl_env.h"
#include "prl_host.h"
#include "prl_obs.h"
#include "prl_rt.h"

namespace {

constexpr int TOBS_THREADS = 256;
constexpr int TOBS_ROW = 33;        // LDS words per row: eb_obs_words' 28 (source words + skip flag), 4 words of action-history bits, 1 pad (odd stride)
constexpr int TOBS_BITS = 28;       // first action-history word of a row
constexpr int TOBS_MAX_HIST_BITS = 128;
constexpr int32_t TOBS_BIT_ENTRY = 1 << 16;  // table entry of an action-history element: TOBS_BIT_ENTRY | bit index

struct TobsFlat {  // FlatLimitPokerEnvBuilder._VEC_ROUND_OFFSETS / _VEC_HALF_ROUND_SIZE per round
    int32_t ofs[4], half[4];
};
struct TobsObs {
    EbFull F;
    uint32_t k0, k1, k2;  // eb_obs_const(0..2)
    int32_t row_dim;
};

PRL_HD PRL_INLINE int tobs_pick4(const int32_t (&a)[4], int r) { return r == 0 ? a[0] : (r == 1 ? a[1] : (r == 2 ? a[2] : a[3])); }

// one tree level: the state after every node's action
PRL_GLOBAL void prl_k_tobs_states(const PrlGame* __restrict__ g, const int32_t* __restrict__ level_nodes, int lo, int n, const int32_t* __restrict__ parent,
                                  const int32_t* __restrict__ action, PrlEnvState* __restrict__ st) {
    const int i = (int)(prl_bid() * prl_nthreads() + prl_tid());
    if (i >= n) return;
    const int node = level_nodes[lo + i], p = parent[node], a = action[node];
    PrlEnvState s;
    if (p < 0) {
        prl_env_reset(*g, s);
    } else {
        s = st[p];
        if (a >= 0) {  // a == -1 below a chance node: the chance outcome keeps its chance parent's post-step state
            PrlStepInfo info;
            prl_env_step(*g, s, a, &info);
        }
    }
    st[node] = s;
}

// one lane per requested node: the compact row list (tree node observed, destination row) of its history, and for Flat its action-history bits
PRL_GLOBAL void prl_k_tobs_paths(const int32_t* __restrict__ parent, const int32_t* __restrict__ kind, const PrlEnvState* __restrict__ st,
                                 const int32_t* __restrict__ req, const int64_t* __restrict__ row_off, const int64_t* __restrict__ cum, int n, int obs_kind,
                                 int invert, TobsFlat fl, int32_t* __restrict__ row_node, int64_t* __restrict__ row_dst, uint32_t* __restrict__ row_bits) {
    const int i = (int)(prl_bid() * prl_nthreads() + prl_tid());
    if (i >= n) return;
    const int node = req[i];
    const int64_t c0 = cum[i];
    if (obs_kind == PRL_OBS_HISTORY) {
        const int64_t T = cum[i + 1] - c0;
        int64_t q = 0;  // decision nodes seen so far, walking up
        for (int v = node; v >= 0; v = parent[v]) {
            if (kind[v] != PRL_NODE_DECISION) continue;
            const int64_t pos = invert ? q : T - 1 - q;
            row_node[c0 + pos] = v;
            row_dst[c0 + pos] = row_off[i] + pos;
            ++q;
        }
        return;
    }
    row_node[c0] = node;
    row_dst[c0] = row_off[i];
    if (obs_kind != PRL_OBS_FLAT_HU_LIMIT) return;
    // _pushback: the action of path node v (its state's last_action: type, seat) was made in the round of the decision node above it and is
    // the count-th action of that seat in that round. Walking up, a node's round is known one decision node later; a first walk counts the
    // actions per (round, seat) (8-bit fields), the second takes each node's count as the number of such actions above it.
    uint64_t tot = 0;
    for (int pass = 0; pass < 2; ++pass) {
        uint32_t b0 = 0u, b1 = 0u, b2 = 0u, b3 = 0u;
        int pa = -1, pla = -1;
        for (int v = node; v >= 0; v = parent[v]) {
            if (kind[v] != PRL_NODE_DECISION) continue;
            const PrlEnvState& s = st[v];
            if (pla >= 0) {
                const int r = s.round, sh = 8 * (2 * r + pa);
                if (pass == 0) {
                    tot += (uint64_t)1 << sh;
                } else {
                    tot -= (uint64_t)1 << sh;
                    const int cnt = (int)((tot >> sh) & 255u);
                    const int idx = tobs_pick4(fl.ofs, r) + pa * tobs_pick4(fl.half, r) + cnt * 2 + pla - 1;
                    const uint32_t bit = (idx >= 0 && idx < TOBS_MAX_HIST_BITS) ? 1u << (idx & 31) : 0u;
                    const int w = idx >> 5;
                    b0 |= w == 0 ? bit : 0u; b1 |= w == 1 ? bit : 0u; b2 |= w == 2 ? bit : 0u; b3 |= w == 3 ? bit : 0u;
                }
            }
            pla = s.last_action[0];
            pa = s.last_action[2];
        }
        if (pass == 1) {
            row_bits[4 * c0 + 0] = b0; row_bits[4 * c0 + 1] = b1; row_bits[4 * c0 + 2] = b2; row_bits[4 * c0 + 3] = b3;
        }
    }
}

// one workgroup per TOBS_THREADS compact rows: each lane puts its row's source words in LDS, then the workgroup writes the rows' floats
// with consecutive lanes on consecutive floats of a row (element m of the workgroup's piece: row m / row_dim, entry m % row_dim)
PRL_GLOBAL void PRL_LAUNCH_BOUNDS(TOBS_THREADS) prl_k_tobs_rows(const PrlGame* __restrict__ g, TobsObs O, const PrlEnvState* __restrict__ st,
                                                                const int32_t* __restrict__ board_id, const int8_t* __restrict__ boards, int board_len,
                                                                const int32_t* __restrict__ row_node, const int64_t* __restrict__ row_dst,
                                                                const uint32_t* __restrict__ row_bits, long long total, float* __restrict__ out) {
    const int T = (int)prl_nthreads(), tid = (int)prl_tid(), D = O.F.obs_dim, RD = O.row_dim;
    char* sm = prl_smem();
    int32_t* tab = (int32_t*)sm;
    uint32_t* rows = (uint32_t*)(sm + (((size_t)RD * 4 + 15) & ~(size_t)15));
    int64_t* dst = (int64_t*)(rows + (((size_t)T * TOBS_ROW + 3) & ~(size_t)3));
    for (int j = tid; j < RD; j += T) tab[j] = j < D ? eb_obs_entry(O.F, j) : (TOBS_BIT_ENTRY | (j - D));
    const long long r0 = (long long)prl_bid() * T;
    const int nr = total - r0 < T ? (int)(total - r0) : T;
    if (tid < nr) {
        const long long k = r0 + tid;
        const int node = row_node[k];
        const PrlEnvState s = st[node];
        const int b = board_id[node], nh2 = 2 * O.F.rules.n_hole_cards;
        int8_t c[16];
#if defined(__clang__)
#pragma unroll
#endif
        for (int d = 0; d < 16; ++d) {  // the env's card row: hole cards (unused here), then the board in deal order
            const int i = d - nh2, ic = i < 0 ? 0 : (i < board_len ? i : board_len - 1);
            const int8_t v = boards[(size_t)(b >= 0 ? b : 0) * board_len + ic];  // always inside the table; kept only where it is a card of the row
            c[d] = (b >= 0 && i >= 0 && i < board_len) ? v : (int8_t)-1;
        }
        const uint32_t k3[3] = {O.k0, O.k1, O.k2};
        uint32_t* w = rows + (size_t)tid * TOBS_ROW;
        eb_obs_words(*g, O.F, s, c, true, k3, w);
        const bool flat = RD > D;
        w[TOBS_BITS + 0] = flat ? row_bits[4 * k + 0] : 0u;
        w[TOBS_BITS + 1] = flat ? row_bits[4 * k + 1] : 0u;
        w[TOBS_BITS + 2] = flat ? row_bits[4 * k + 2] : 0u;
        w[TOBS_BITS + 3] = flat ? row_bits[4 * k + 3] : 0u;
        dst[tid] = row_dst[k];
    }
    prl_sync();
    const int n_el = nr * RD, de = T / RD, dj = T % RD;
    int e = tid / RD, j = tid % RD;
    for (int m = tid; m < n_el; m += T) {
        const int32_t t = tab[j];
        const uint32_t* R = rows + (size_t)e * TOBS_ROW;
        uint32_t u;
        if (t & TOBS_BIT_ENTRY) {
            const int bi = t & 0xFFFF;
            u = ((R[TOBS_BITS + (bi >> 5)] >> (bi & 31)) & 1u) ? 0x3F800000u : 0u;
        } else {
            const uint32_t wv = R[t & 255];
            const int cm = t >> 8;
            u = cm ? ((int)wv == cm - 1 ? 0x3F800000u : 0u) : wv;
        }
        float v;
        __builtin_memcpy(&v, &u, 4);
        out[dst[e] * RD + j] = v;
        e += de; j += dj;
        if (j >= RD) { j -= RD; ++e; }
    }
}

// legal[i][a] = 1 if action int a is a child of requested node i: one lane per byte
PRL_GLOBAL void prl_k_tobs_legal(const int32_t* __restrict__ req, const int32_t* __restrict__ first_col, const int32_t* __restrict__ n_children,
                                 const int32_t* __restrict__ col_action, long long n_bytes, int n_actions, uint8_t* __restrict__ legal) {
    const long long i = (long long)prl_bid() * prl_nthreads() + prl_tid();
    if (i >= n_bytes) return;
    const long long r = i / n_actions;
    const int a = (int)(i - r * n_actions), node = req[r], c0 = first_col[node], nc = n_children[node];
    uint8_t v = 0;
    for (int q = 0; q < nc; ++q) v |= col_action[c0 + q] == a ? 1 : 0;
    legal[i] = v;
}

}  // namespace

struct PrlTreeObs {
    std::vector<int32_t> dlen;    // host: decision nodes on the root path of every node, itself included
    bool states_ready = false;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    PrlGame* d_game = nullptr;
    PrlEnvState* d_state = nullptr;
    int32_t* d_ints = nullptr;    // parent, action, kind, board_id, first_col, n_children, level_nodes [n_nodes each], col_action [n_cols]
    int8_t* d_boards = nullptr;
    char* d_scratch = nullptr;    // per call: requests, offsets, the compact row list
    size_t scratch_bytes = 0;
    double state_bytes = 0, states_ms = 0, obs_ms = 0, obs_bytes = 0;
};

void prl_tree_obs_free(PrlTreeObs* c) {
    if (!c) return;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    void* ptrs[] = {c->d_game, c->d_state, c->d_ints, c->d_boards, c->d_scratch};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

static PrlTreeObs* tobs_host(const prl_tree_t* tree) {
    if (!tree->obs) {
        const PrlFlatTree& t = tree->t;
        PrlTreeObs* c = new PrlTreeObs();
        c->dlen.resize(t.n_nodes);
        for (int i = 0; i < t.n_nodes; ++i)  // DFS pre-order: a parent precedes its children
            c->dlen[i] = (t.parent[i] >= 0 ? c->dlen[t.parent[i]] : 0) + (t.kind[i] == PRL_NODE_DECISION ? 1 : 0);
        tree->obs = c;
    }
    return tree->obs;
}

// the device half, made on first use: the tree's arrays in HBM and the env state of every node (one launch per level)
static int32_t tobs_device(const prl_tree_t* tree, PrlTreeObs* c) {
    if (c->states_ready) return PRL_OK;
    const PrlFlatTree& t = tree->t;
    const size_t nn = (size_t)t.n_nodes;
    if (!c->stream) {
        PRL_HIP_TRY(hipStreamCreate(&c->stream));
        for (hipEvent_t& e : c->ev) PRL_HIP_TRY(hipEventCreate(&e));
    }
    if (!c->d_game) PRL_HIP_TRY(hipMalloc((void**)&c->d_game, sizeof(PrlGame)));
    if (!c->d_state) PRL_HIP_TRY(hipMalloc((void**)&c->d_state, nn * sizeof(PrlEnvState)));
    if (!c->d_ints) PRL_HIP_TRY(hipMalloc((void**)&c->d_ints, (7 * nn + (size_t)t.n_cols) * sizeof(int32_t)));
    if (!c->d_boards) PRL_HIP_TRY(hipMalloc((void**)&c->d_boards, t.boards.size() ? t.boards.size() : 1));
    c->state_bytes = (double)nn * sizeof(PrlEnvState);
    PRL_HIP_TRY(hipMemcpyAsync(c->d_game, &t.game, sizeof(PrlGame), hipMemcpyHostToDevice, c->stream));
    const std::vector<int32_t>* arrs[] = {&t.parent, &t.action, &t.kind, &t.board_id, &t.first_col, &t.n_children, &t.level_nodes};
    for (int k = 0; k < 7; ++k) PRL_HIP_TRY(hipMemcpyAsync(c->d_ints + k * nn, arrs[k]->data(), nn * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (t.n_cols) PRL_HIP_TRY(hipMemcpyAsync(c->d_ints + 7 * nn, t.col_action.data(), (size_t)t.n_cols * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (t.boards.size()) PRL_HIP_TRY(hipMemcpyAsync(c->d_boards, t.boards.data(), t.boards.size(), hipMemcpyHostToDevice, c->stream));
    PRL_HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    for (int d = 0; d < t.n_levels; ++d) {
        const int lo = t.level_start[d], n = t.level_start[d + 1] - lo;
        if (n > 0)
            PRL_LAUNCH(prl_k_tobs_states, (n + TOBS_THREADS - 1) / TOBS_THREADS, TOBS_THREADS, 0, c->stream, (const PrlGame*)c->d_game,
                       (const int32_t*)(c->d_ints + 6 * nn), lo, n, (const int32_t*)c->d_ints, (const int32_t*)(c->d_ints + nn), c->d_state);
    }
    PRL_HIP_TRY(hipGetLastError());
    PRL_HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    PRL_HIP_TRY(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    PRL_HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    c->states_ms = ms;
    c->states_ready = true;
    return PRL_OK;
}

static bool tobs_decision(const PrlFlatTree& t, int32_t idx) {
    return idx >= 0 && idx < t.n_nodes && t.kind[idx] == PRL_NODE_DECISION && t.n_children[idx] > 0;
}

extern "C" int32_t prl_tree_obs_hist_len(const prl_tree_t* tree, const int32_t* node_idx, int32_t n, int32_t* out_hist_len) {
    if (!tree || n < 0 || (n > 0 && (!node_idx || !out_hist_len))) { prl_set_error("prl_tree_obs_hist_len: bad argument"); return PRL_ERR_ARG; }
    const PrlFlatTree& t = tree->t;
    if (t.is_partial) { prl_set_error("prl_tree_obs_hist_len: partial tree"); return PRL_ERR_ARG; }
    for (int32_t i = 0; i < n; ++i)
        if (!tobs_decision(t, node_idx[i])) { prl_set_error("prl_tree_obs_hist_len: node " + std::to_string(node_idx[i]) + " is not a decision node of the tree"); return PRL_ERR_ARG; }
    const PrlTreeObs* c = tobs_host(tree);
    for (int32_t i = 0; i < n; ++i) out_hist_len[i] = c->dlen[node_idx[i]];
    return PRL_OK;
}

extern "C" int32_t prl_tree_observations_device(const prl_tree_t* tree, int32_t kind, int32_t invert, const int32_t* node_idx, const int64_t* row_offset,
                                                int32_t n, const int32_t* flat_offsets, int32_t row_dim, int64_t n_rows, float* d_out, uint8_t* d_legal,
                                                int32_t n_actions) {
    auto bad = [](const std::string& why) { prl_set_error("prl_tree_observations_device: " + why); return PRL_ERR_ARG; };
    if (!tree) return bad("NULL tree");
    const PrlFlatTree& t = tree->t;
    if (t.is_partial) return bad("partial tree (stop_at_street): its nodes below the limit have no observations here");
    if (kind != PRL_OBS_VANILLA && kind != PRL_OBS_HISTORY && kind != PRL_OBS_FLAT_HU_LIMIT) return bad("unknown kind");
    if (n < 0 || n_rows < 0 || (n > 0 && (!node_idx || !row_offset || !d_out))) return bad("NULL or negative argument");
    if (t.rules.n_hole_cards * 2 + t.rules.n_board_cards > 16 || t.rules.n_rounds > 4) return bad("unsupported game shape");
    const int D = eb_obs_dim(t.rules);
    TobsFlat fl;
    for (int r = 0; r < 4; ++r) { fl.ofs[r] = 0; fl.half[r] = 0; }
    if (kind == PRL_OBS_FLAT_HU_LIMIT) {
        if (t.game.game_type != PRL_GAME_LIMIT) return bad("the flat action-history observation is for fixed-limit games");
        if (!flat_offsets) return bad("flat_offsets is NULL");
        const int V = row_dim - D;
        int sum = 0;
        for (int r = 0; r < t.rules.n_rounds; ++r) {
            fl.ofs[r] = flat_offsets[r];
            fl.half[r] = flat_offsets[t.rules.n_rounds + r];
            if (fl.ofs[r] < 0 || fl.half[r] < 0 || fl.ofs[r] + 2 * fl.half[r] > V) return bad("flat_offsets outside the action vector");
            sum += 2 * fl.half[r];
        }
        if (V <= 0 || V > TOBS_MAX_HIST_BITS || V != sum) return bad("row_dim is not obs_dim + the action vector (at most 128 entries)");
    } else if (row_dim != D) {
        return bad("row_dim " + std::to_string(row_dim) + " != the observation's " + std::to_string(D));
    }
    if (d_legal) {
        const int n_act = t.game.game_type == PRL_GAME_DISCRETIZED ? t.game.n_bet_sizes + 2 : 3;
        if (n_actions < n_act) return bad("n_actions is smaller than the game's");
    }
    PrlTreeObs* c = tobs_host(tree);
    std::vector<int64_t> cum((size_t)n + 1, 0);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t idx = node_idx[i];
        if (!tobs_decision(t, idx)) return bad("node " + std::to_string(idx) + " is not a decision node of the tree");
        const int64_t rows = kind == PRL_OBS_HISTORY ? c->dlen[idx] : 1;
        if (row_offset[i] < 0 || row_offset[i] > n_rows - rows) return bad("the rows of request " + std::to_string(i) + " overrun n_rows");
        cum[i + 1] = cum[i] + rows;
    }
    const int64_t total = cum[n];
    c->obs_ms = 0;
    c->obs_bytes = 0;
    if (n == 0) return PRL_OK;
    int32_t rc = tobs_device(tree, c);
    if (rc) return rc;
    // scratch: requests, row offsets, cum, then the compact row list (node, destination row, Flat's four bit words)
    auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t b_req = al((size_t)n * 4), b_off = al((size_t)n * 8), b_cum = al(((size_t)n + 1) * 8), b_node = al((size_t)total * 4),
                 b_dst = al((size_t)total * 8), b_bits = kind == PRL_OBS_FLAT_HU_LIMIT ? al((size_t)total * 16) : 16;
    const size_t need = b_req + b_off + b_cum + b_node + b_dst + b_bits;
    if (need > c->scratch_bytes) {
        if (c->d_scratch) { PRL_HIP_TRY(hipStreamSynchronize(c->stream)); (void)hipFree(c->d_scratch); c->d_scratch = nullptr; c->scratch_bytes = 0; }
        PRL_HIP_TRY(hipMalloc((void**)&c->d_scratch, need));
        c->scratch_bytes = need;
    }
    char* p = c->d_scratch;
    int32_t* d_req = (int32_t*)p; p += b_req;
    int64_t* d_off = (int64_t*)p; p += b_off;
    int64_t* d_cum = (int64_t*)p; p += b_cum;
    int32_t* d_node = (int32_t*)p; p += b_node;
    int64_t* d_dst = (int64_t*)p; p += b_dst;
    uint32_t* d_bits = (uint32_t*)p;
    PRL_HIP_TRY(hipMemcpyAsync(d_req, node_idx, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    PRL_HIP_TRY(hipMemcpyAsync(d_off, row_offset, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    PRL_HIP_TRY(hipMemcpyAsync(d_cum, cum.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    const size_t nn = (size_t)t.n_nodes;
    const int32_t *d_parent = c->d_ints, *d_kind = c->d_ints + 2 * nn, *d_board_id = c->d_ints + 3 * nn, *d_first_col = c->d_ints + 4 * nn,
                  *d_n_children = c->d_ints + 5 * nn, *d_col_action = c->d_ints + 7 * nn;
    TobsObs O;
    O.F.rules = t.rules;
    O.F.n_deal = 2 * t.rules.n_hole_cards + t.rules.n_board_cards;
    O.F.obs_dim = D;
    O.F.suits_matter = t.rules.rank_rule == 2 ? 1 : 0;  // game_rules.py: SUITS_MATTER (as eb_full)
    O.F.reward_scalar = 1.0;
    O.k0 = eb_obs_const(t.game, 0); O.k1 = eb_obs_const(t.game, 1); O.k2 = eb_obs_const(t.game, 2);
    O.row_dim = row_dim;
    const size_t smem = (((size_t)row_dim * 4 + 15) & ~(size_t)15) + (((size_t)TOBS_THREADS * TOBS_ROW + 3) & ~(size_t)3) * 4 + (size_t)TOBS_THREADS * 8;
    PRL_HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    PRL_LAUNCH(prl_k_tobs_paths, (n + TOBS_THREADS - 1) / TOBS_THREADS, TOBS_THREADS, 0, c->stream, d_parent, d_kind, (const PrlEnvState*)c->d_state,
               (const int32_t*)d_req, (const int64_t*)d_off, (const int64_t*)d_cum, (int)n, (int)kind, invert ? 1 : 0, fl, d_node, d_dst, d_bits);
    PRL_LAUNCH(prl_k_tobs_rows, (unsigned)((total + TOBS_THREADS - 1) / TOBS_THREADS), TOBS_THREADS, smem, c->stream, (const PrlGame*)c->d_game, O,
               (const PrlEnvState*)c->d_state, d_board_id, (const int8_t*)c->d_boards, t.board_len, (const int32_t*)d_node, (const int64_t*)d_dst,
               (const uint32_t*)d_bits, (long long)total, d_out);
    if (d_legal) {
        const long long nb = (long long)n * n_actions;
        PRL_LAUNCH(prl_k_tobs_legal, (unsigned)((nb + TOBS_THREADS - 1) / TOBS_THREADS), TOBS_THREADS, 0, c->stream, (const int32_t*)d_req, d_first_col,
                   d_n_children, d_col_action, nb, (int)n_actions, d_legal);
    }
    PRL_HIP_TRY(hipGetLastError());
    PRL_HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    PRL_HIP_TRY(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    PRL_HIP_TRY(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
    c->obs_ms = ms;
    c->obs_bytes = (double)total * row_dim * 4 + (d_legal ? (double)n * n_actions : 0.0);
    return PRL_OK;
}

extern "C" int32_t prl_tree_obs_stats(const prl_tree_t* tree, double* out) {
    if (!tree || !out) { prl_set_error("prl_tree_obs_stats: bad argument"); return PRL_ERR_ARG; }
    const PrlTreeObs* c = tree->obs;
    out[0] = c ? c->state_bytes : 0.0;
    out[1] = c ? c->states_ms : 0.0;
    out[2] = c ? c->obs_ms : 0.0;
    out[3] = c ? c->obs_bytes : 0.0;
    return PRL_OK;
}

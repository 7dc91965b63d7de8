// Board-pass kernel of the fused engine, included once per registered board-subtree shape by prl_fhp_kernels.hip inside a
// namespace. Expects FHP_THREADS, FHP_SLOTS, FHP_LAUNCH_BOUNDS and FHP_SPEC (the shape's spec struct, prl_fhp.h) to be defined.
//
// One workgroup walks one board subtree. SORTED STORAGE (prl_fhp.h): a lane owns two ADJACENT RANK-SORTED POSITIONS of the board (not two
// hands) and the board's columns are stored in that order, so "hand-local" below means "position-local": the lane's writes into the sorted
// domain (phase B), its reads at its own position (phase E) and its column loads / stores are linear; only the tie-group bounds (E), the
// per-card lists (C) and the per-card totals (E) are gathers. Per seat p (two "batches" per board):
//   B  top-down, hand-local: the opponent's reach at the 9 terminals -> LDS (the lane's own two positions of every vector)
//   C  per-card blocker scans of all 9 vectors in the row16 order (prl_device.h): a row of 16 lanes owns one card's list, 3
//      entries per lane, so the 12 waves take the 47 live cards in ONE round; corrections K (showdown; the lower card of a
//      hand stores, the higher card's value waits in registers and is added after the phase barrier) and per-card totals (fold)
//   D  range prefix of every vector (one wave per vector, chunk carries in a register), written IN PLACE over the vector
//   E  bottom-up, hand-local: terminal values from LDS, seat p's EV (and best response) up to the board root, and -- if p
//      is the seat being updated -- its new regrets, new strategy and CFR+ running average straight to HBM; in
//      UPDATE1_EVAL1 a second phase E then plays the new strategy (prl_fhp.h: pass modes)
// While a board is being walked, the NEXT board's regrets and plan stream from HBM into an LDS prefetch area with the
// gfx950 LDS-DMA loads (no registers, no waiting): the board start reads LDS instead of paying an HBM round trip with
// the whole workgroup stalled. All barriers order LDS traffic only, so they do not drain the DMA.
#ifndef FHP_NPAD
#define FHP_NPAD 1088  // >= 1081 live hands of a 5-card board, multiple of 64
#define FHP_NLIVE 1081  // C(47, 2): hands that do not hold a board card, the same number for every board
#define FHP_NCARDS 52
#define FHP_R 1326     // hands of a 52-card deck (the launcher rejects any other range size)
#define FHP_NP PRL_FHP_NP  // elements per board column in HBM (sorted storage) = FHP_NPAD
#define FHP_NSHOW (PrlFhpShape::N_SHOW)   // showdown / fold terminals of the shape this file is being instantiated for
#define FHP_NFOLD (PrlFhpShape::N_FOLD)
#define FHP_NVEC (PrlFhpShape::N_SHOW + PrlFhpShape::N_FOLD)
#endif
typedef PrlFhpDerive<FHP_SPEC> PrlFhpShape;
// FHP_EXPERIMENT builds (scripts/gpu_toggle.py): a run-time switch (PrlFhpParams::exp) between two code paths of ONE solver -- the only
// A/B that is not drowned by the allocation-to-allocation spread of the board pass (profiles/r02_experiments.txt)
#if defined(FHP_EXPERIMENT)
#define FHP_EXP(c, bit) (((c).prm->exp & (bit)) != 0)
#define FHP_AVG_PIPELINED(c) true
#define FHP_TERMINAL_CACHE(c) true  // (set one of these to FHP_EXP(c, bit) to toggle that path in an experiment build)
#else
#define FHP_EXP(c, bit) false
#define FHP_AVG_PIPELINED(c) true
#define FHP_TERMINAL_CACHE(c) true
#endif
static_assert(PrlFhpShape::subtree_size(0) == PrlFhpShape::N_NODES, "the spec is one DFS pre-order tree");
static_assert(FHP_NP == FHP_NPAD && FHP_NP == PRL_PP_NPAD && FHP_R == PRL_PP_R && FHP_SLOTS == 2, "sorted storage: a column holds the padded sorted domain, a lane two positions");

#include "prl_fhp_div.inc"
struct FhpV { FhpF v; };

// A loop over the action columns whose index is a COMPILE-TIME constant inside the body. The shape derivations (PrlFhpDerive:
// col_actor, col0, folder ...) are nested loops over the listing; asked with a run-time index inside a `#pragma unroll` loop they are
// constant-folded on the 9- and 15-node shapes but survive as scalar code on the 21-node one (200-400 scalar branches per kernel,
// measured on the per-street engine's 27-node shape as 17x the whole pass: profiles/r05_experiments.txt). Hence template recursion.
template <int I, int N, class F>
PRL_DEV PRL_INLINE void fhp_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>());
        fhp_static_for<I + 1, N>(f);
    }
}
template <int J, class F>
PRL_DEV PRL_INLINE void fhp_for_cols(F&& f) {
    if constexpr (J < PrlFhpShape::N_COLS) {
        f(std::integral_constant<int, J>());
        fhp_for_cols<J + 1>(f);
    }
}

// A lane owns the FHP_SLOTS adjacent hands tid * FHP_SLOTS + k. With two slots its global accesses are one 8-byte
// (float) or 16-byte (double) instruction; every column / vector base is a multiple of R = 1326 (even) elements from a
// 16-byte aligned allocation, so the pairs are naturally aligned.
template <class T> struct alignas(2 * sizeof(T)) FhpPair { T a, b; };
template <class T>
PRL_DEV PRL_INLINE void fhp_gload(const T* p, T (&out)[FHP_SLOTS]) {
    if constexpr (FHP_SLOTS == 2) { const FhpPair<T> v = *(const FhpPair<T>*)p; out[0] = v.a; out[1] = v.b; }
    else { for (int k = 0; k < FHP_SLOTS; ++k) out[k] = p[k]; }
}
template <class T>
PRL_DEV PRL_INLINE void fhp_gstore(T* p, const T (&in)[FHP_SLOTS]) {
    if constexpr (FHP_SLOTS == 2) { FhpPair<T> v; v.a = in[0]; v.b = in[1]; *(FhpPair<T>*)p = v; }
    else { for (int k = 0; k < FHP_SLOTS; ++k) p[k] = in[k]; }
}
// streaming variants (nontemporal: the line is not kept in L2): regrets / averages written now are next read a whole iteration later.
// Run-time toggle on one solver: stores alone -0.16 %, the average's loads alone +1.6 %, both -0.7 % (5 solvers, consistent)
template <class T>
PRL_DEV PRL_INLINE void fhp_gstore_nt(T* p, const T (&in)[FHP_SLOTS]) {
#if defined(PRL_EMU)
    fhp_gstore(p, in);
#else
    if constexpr (FHP_SLOTS == 2 && sizeof(T) == 4) {
        typedef float v2 __attribute__((ext_vector_type(2)));
        v2 v; v.x = in[0]; v.y = in[1];
        __builtin_nontemporal_store(v, (v2*)p);
    } else if constexpr (FHP_SLOTS == 2 && sizeof(T) == 8) {
        typedef double d2 __attribute__((ext_vector_type(2)));
        d2 v; v.x = in[0]; v.y = in[1];
        __builtin_nontemporal_store(v, (d2*)p);
    } else { for (int k = 0; k < FHP_SLOTS; ++k) __builtin_nontemporal_store(in[k], p + k); }
#endif
}
template <class T>
PRL_DEV PRL_INLINE void fhp_gload_nt(const T* p, T (&out)[FHP_SLOTS]) {
#if defined(PRL_EMU)
    fhp_gload(p, out);
#else
    if constexpr (FHP_SLOTS == 2 && sizeof(T) == 8) {
        typedef double d2 __attribute__((ext_vector_type(2)));
        const d2 v = __builtin_nontemporal_load((const d2*)p);
        out[0] = v.x; out[1] = v.y;
    } else if constexpr (FHP_SLOTS == 2 && sizeof(T) == 4) {
        typedef float v2 __attribute__((ext_vector_type(2)));
        const v2 v = __builtin_nontemporal_load((const v2*)p);
        out[0] = v.x; out[1] = v.y;
    } else { for (int k = 0; k < FHP_SLOTS; ++k) out[k] = __builtin_nontemporal_load(p + k); }
#endif
}
PRL_DEV PRL_INLINE void fhp_gstore(float* p, const FhpF& in) {
    float t[FHP_SLOTS];
    for (int k = 0; k < FHP_SLOTS; ++k) t[k] = in[k];
    fhp_gstore(p, t);
}

// the lane's two adjacent positions of a PLANAR LDS vector as ONE 8-byte access (p0 is even, every vector starts 8-byte aligned)
PRL_DEV PRL_INLINE FhpF fhp_lds_load2(const float* v, int p0) { return *(const FhpF*)(v + p0); }
PRL_DEV PRL_INLINE void fhp_lds_store2(float* v, int p0, const FhpF& x) { *(FhpF*)(v + p0) = x; }

// PAIR-INTERLEAVED terminal vectors (round 5). The per-card scans (phase C) gather every terminal vector at the same three positions per lane: with
// planar vectors that is NVEC 4-byte gathers per entry, and a ds_read_b32 moves 128 bytes per clock where ds_read_b64 moves 256 (MI355X_MICROARCH.md,
// LDS: 32 banks against 64) -- the gathers were the biggest LDS item of the pass. Vectors 2j and 2j+1 therefore share one array [NPAD][2]: element
// (v, q) sits at word fhp_y_base(v) + fhp_y_step(v) * q, one 8-byte gather fetches both. An odd last vector stays planar, so the area is
// NVEC * NPAD words as before. The position-local phases pay for it with wider accesses at their own two positions: a 16-byte store per pair in
// phase B, a 16-byte read where phase E wants its own value of a fold vector; the range prefix (phase D, a wave per vector) walks its vector with a
// stride of two words (two lanes per bank: free on a store, one extra LDS cycle on a 4-byte read).
// Which two vectors share an array follows the ORDER OF THE WALK: vector u of the gather array is the u-th terminal in DFS order (fhp_yord(slot)), so
// phase B holds a terminal's reach for one more terminal at most before the pair is stored (collecting all of them first cost 20 registers).
#define FHP_NPAIRS (FHP_NVEC / 2)
constexpr int fhp_y_base(int u) { return u < 2 * FHP_NPAIRS ? (u >> 1) * (2 * FHP_NPAD) + (u & 1) : 2 * FHP_NPAIRS * FHP_NPAD; }
constexpr int fhp_y_step(int u) { return u < 2 * FHP_NPAIRS ? 2 : 1; }
constexpr int fhp_term_node(int slot) {
    for (int n = 0; n < PrlFhpShape::N_NODES; ++n)
        if (PrlFhpShape::kind(n) != PRL_NODE_DECISION && PrlFhpShape::term_slot(n) == slot) return n;
    return -1;
}
constexpr int fhp_yord(int slot) {  // rank of the slot's terminal among all terminals in DFS (= node id) order
    int u = 0;
    for (int n = 0; n < fhp_term_node(slot); ++n) u += PrlFhpShape::kind(n) != PRL_NODE_DECISION;
    return u;
}
constexpr unsigned fhp_show_mask() {  // bit u: vector u of the gather array belongs to a showdown terminal
    unsigned m = 0;
    for (int s = 0; s < PrlFhpShape::N_SHOW; ++s) m |= 1u << fhp_yord(s);
    return m;
}
#if defined(PRL_EMU)
struct FhpQ { float e[4]; float& operator[](int k) { return e[k]; } const float& operator[](int k) const { return e[k]; } };
#else
typedef float FhpQ __attribute__((ext_vector_type(4)));
#endif

// PRL_FHP_TIMING builds (scripts/gpu_phases.sh): wave 0 accumulates the shader clock spent between phase boundaries
#ifdef PRL_FHP_TIMING
// (accumulated in registers, one atomic per phase at the end of the kernel: 256 workgroups hitting eight words after every phase saturate them)
#define FHP_TICK(c, i) do { const long long t_ = __builtin_readcyclecounter(); (c).t_acc[i] += t_ - (c).t_prev; (c).t_prev = t_; } while (0)
// per-wave waiting time at each of the five barriers of a seat's batch: timing[8 + 12 * barrier + wave]
#ifdef PRL_FHP_TIMING_BARRIERS  // (every wave's atomics at every barrier: slows the pass ~6x -- for the relative waiting times only)
#define FHP_SYNC(c, id) do { const long long a_ = clock64(); prl_sync_lds(); if ((prl_tid() & 63) == 0) atomicAdd((c).prm->timing + 8 + 12 * (id) + (prl_tid() >> 6), (unsigned long long)(clock64() - a_)); } while (0)
#else
#define FHP_SYNC(c, id) prl_sync_lds()
#endif
#else
#define FHP_TICK(c, i) do { } while (0)
#define FHP_SYNC(c, id) prl_sync_lds()
#endif

struct FhpLds {
    float* y;       // [9][NPAD]  opponent reach at the terminals, sorted domain (showdown 0..4, fold 5..8), PAIR-INTERLEAVED (fhp_y_base / fhp_y_step);
                    //            the showdown vectors are overwritten in phase D by Pm[j] = P[j + 1]
    float* K;       // [2][5][NPAD]  blocker corrections per sorted position (showdown): K_c of the hand's lower card, then of its higher card
    float* Tc;      // [4][64]    per-card totals (fold)
    float* Tt;      // [16]       range totals P[n_live] of the terminal vectors
    // prefetch area (next board), filled by 16-byte LDS DMA from the 16-byte aligned address at or below the source:
    // element i of a source lands at word fhp_lead(source) + i of its area
    float* pf_rg;       // the first opponent's regret columns, run by run (fhp_run_*)
    uint32_t* pf_clx;   // [768][2] per-lane records of the per-card scans (prl_solver_types.h: PRL_CLX_*)
    uint32_t* pf_pp;    // [PRL_PP_STRIDE / 2] the position-domain plan (int16 pairs as dwords: PRL_PP_*)
    float* acc;         // [out width][R] running sums of the current block's root vectors, HAND order (block_sum)
};
PRL_DEV PRL_INLINE int fhp_lead(const void* p) { return (int)(((size_t)p >> 2) & 3); }  // words between the aligned address and p
// a prefetch area holds WHOLE rows (64 lanes x 16 bytes = 256 words): every DMA instruction runs with all lanes on, the tail of the
// last row reads on into the next board's data (the allocations are padded at the far end) and lands in the area's padding
#define FHP_PF_ROWS(words) ((((words) + 3 + 3) / 4 + 63) / 64)
#define FHP_PF_AREA(words) (FHP_PF_ROWS(words) * 256)
#define FHP_PP_WORDS (PRL_PP_STRIDE / 2)
#define FHP_ACC_WORDS (4 * FHP_R)  // the widest row (EVAL: both seats' values and best responses)
// OPPONENT-ONLY regret prefetch (round 5). Of a board's [N_COLS][NP] float32 block only the columns of the seat whose reach the FIRST batch walks
// (phase B needs them the moment the board starts) come through the LDS prefetch area; the other seat's columns are needed in phase E at the
// earliest and are requested from HBM at the board start, three phases of cover ahead. A seat's columns lie in RUNS of adjacent columns (a
// decision node's columns are adjacent; FHP15: seat 1 = {0,1} {4,5,6} {12,13}, seat 0 = {2,3} {7..11}); a run is one DMA segment of whole rows.
constexpr bool fhp_run_starts(int seat, int j) { return PrlFhpShape::col_actor(j) == seat && (j == 0 || PrlFhpShape::col_actor(j - 1) != seat); }
constexpr int fhp_n_runs(int seat) { int n = 0; for (int j = 0; j < PrlFhpShape::N_COLS; ++j) n += fhp_run_starts(seat, j); return n; }
constexpr int fhp_run_col0(int seat, int r) {
    for (int j = 0, n = 0; j < PrlFhpShape::N_COLS; ++j)
        if (fhp_run_starts(seat, j) && n++ == r) return j;
    return PrlFhpShape::N_COLS;
}
constexpr int fhp_run_cols(int seat, int r) {
    int n = 0;
    for (int j = fhp_run_col0(seat, r); j < PrlFhpShape::N_COLS && PrlFhpShape::col_actor(j) == seat; ++j) ++n;
    return n;
}
constexpr int fhp_run_rows(int seat, int r) { return FHP_PF_ROWS(fhp_run_cols(seat, r) * FHP_NP); }
constexpr int fhp_run_row0(int seat, int r) { int s = 0; for (int i = 0; i < r; ++i) s += fhp_run_rows(seat, i); return s; }
constexpr int fhp_seat_rows(int seat) { return fhp_run_row0(seat, fhp_n_runs(seat)); }
constexpr int fhp_col_run(int j) {  // the run (of its seat) that holds column j
    const int seat = PrlFhpShape::col_actor(j);
    for (int r = 0; r < fhp_n_runs(seat); ++r)
        if (fhp_run_col0(seat, r) <= j && j < fhp_run_col0(seat, r) + fhp_run_cols(seat, r)) return r;
    return -1;
}
constexpr int FHP_PF_RG_ROWS = fhp_seat_rows(0) > fhp_seat_rows(1) ? fhp_seat_rows(0) : fhp_seat_rows(1);
#define FHP_PF_RG_WORDS (FHP_PF_RG_ROWS * 256)
#define FHP_LDS_WORK_BYTES ((FHP_NVEC * FHP_NPAD + 2 * FHP_NSHOW * FHP_NPAD + FHP_NFOLD * 64 + 16 + FHP_ACC_WORDS) * 4)
#define FHP_LDS_BYTES_WITH_RG (FHP_LDS_WORK_BYTES + (FHP_PF_RG_WORDS + FHP_PF_AREA(PRL_CLX_WORDS) + FHP_PF_AREA(FHP_PP_WORDS)) * 4)
// shapes whose opponent columns do not fit beside the work area stream the plan only and read all their regrets straight from HBM
// at the board start (one exposed round trip per board instead of none)
#define FHP_RG_IN_LDS (FHP_LDS_BYTES_WITH_RG <= 160 * 1024)
#define FHP_LDS_BYTES (FHP_RG_IN_LDS ? FHP_LDS_BYTES_WITH_RG : FHP_LDS_BYTES_WITH_RG - FHP_PF_RG_WORDS * 4)

PRL_DEV PRL_INLINE FhpLds fhp_lds() {
    FhpLds L;
    float* f = (float*)prl_smem();
    L.y = f; f += FHP_NVEC * FHP_NPAD;
    L.K = f; f += 2 * FHP_NSHOW * FHP_NPAD;
    L.Tc = f; f += FHP_NFOLD * 64;
    L.Tt = f; f += 16;
    L.acc = f; f += FHP_ACC_WORDS;
    L.pf_rg = f; f += FHP_RG_IN_LDS ? FHP_PF_RG_WORDS : 0;
    L.pf_clx = (uint32_t*)f; f += FHP_PF_AREA(PRL_CLX_WORDS);
    L.pf_pp = (uint32_t*)f; f += FHP_PF_AREA(FHP_PP_WORDS);
    return L;
}

// STEADY = the steady state of CFR+ (prl_fhp_steady_plus: variant CFR+, not the first iteration, running average being blended,
// no Vanilla / Linear sum riding on the walk): the wave-uniform run-time switches below are compile-time constants, which removes
// their scalar tests, the dead sides of every select and the SGPRs that held them (a clamp r > 0 ? r : 0 on regrets that CFR+
// already stores clamped costs three instructions per regret otherwise).
//
// PAIRED AVERAGE UPDATES (PrlFhpParams::avg_pair). The CFR+ average is a scalar-weighted recurrence, a_t = m_old_t * a_(t-1) + m_new_t * s_t, and the
// strategy s_t that enters it -- regret matching of the regrets iteration t stores -- is recomputed by the pass of iteration t + 1 anyway (it plays
// it). So of a pair (t, t + 1) inside one prl_solver_iterations call, t leaves the board average alone (DEFERRED: no old-average loads, no new-strategy
// divisions where nothing else needs them, no average stores) and t + 1 applies both steps in registers (CATCH-UP: the node's old strategy s[i][k],
// already there for the EV, with iteration t's weights, then its own step): the same operations in the same order with the same roundings, one HBM
// round trip of the float64 columns instead of two. STEADY 5 / 6 are the two as compile-time kinds; the generic instantiation asks at run time.
//
// SPLIT PAIRS (PrlFhpParams::avg_pair_b). The recurrence is per column, so nothing forces all of a seat's columns into the same pair phase: a seat's
// decision nodes are split at compile time into set A and set B (fhp_avg_set: balanced column counts), B's pairs run one iteration behind A's, and every
// launch of a long call carries the float64 round trip of about half a seat's columns instead of all (catch-up) or none (deferred) of them. The steady
// kind is then a PAIR (kind of A, kind of B) of 1 (unpaired) / 5 (deferred) / 6 (catch-up), STEADY = fhp_steady_pair(ka, kb); equal kinds are the
// whole-board kinds 1 / 5 / 6 themselves. Which nodes load and store an average is a compile-time property of (STEADY, node) in every steady kind.
constexpr int FHP_STEADY_PAIR0 = 16;
constexpr int fhp_kind_code(int k) { return k == 1 ? 0 : k == 5 ? 1 : 2; }
constexpr int fhp_steady_pair(int ka, int kb) { return ka == kb ? ka : FHP_STEADY_PAIR0 + 4 * fhp_kind_code(ka) + fhp_kind_code(kb); }
constexpr int fhp_code_kind(int c) { return c == 0 ? 1 : c == 1 ? 5 : 6; }
constexpr int fhp_set_kind(int steady, int set) {  // the kind that the nodes of set 0 (A) / 1 (B) run under
    return steady < FHP_STEADY_PAIR0 ? steady : fhp_code_kind(set == 0 ? (steady - FHP_STEADY_PAIR0) / 4 : (steady - FHP_STEADY_PAIR0) % 4);
}
constexpr bool fhp_steady_plus(int steady) { return steady == 1 || steady == 4 || steady == 5 || steady == 6 || steady >= FHP_STEADY_PAIR0; }
// Set of a decision node, 0 = A, 1 = B: the seat's nodes by falling action count (DFS order among equals), each into the set that holds fewer columns
// so far, B on a tie. FHP15: per seat 2 + 2 + 3 columns, A = the two two-action nodes, B = the three-action node; FHP9 2 | 2; FHP21 5 | 5.
constexpr int fhp_avg_set(int n) {
    int cols[2] = {0, 0};
    for (int a = PrlFhpShape::MAX_A; a >= 1; --a)
        for (int m = 0; m < PrlFhpShape::N_NODES; ++m)
            if (PrlFhpShape::kind(m) == PRL_NODE_DECISION && PrlFhpShape::actor(m) == PrlFhpShape::actor(n) && PrlFhpShape::nch(m) == a) {
                const int set = cols[1] <= cols[0] ? 1 : 0;
                if (m == n) return set;
                cols[set] += a;
            }
    return 0;
}
// does decision node n load (and store) a blended average under this kind? The generic kind may: it asks at run time.
constexpr bool fhp_may_load_avg(int steady, int n) {
    if (steady == 0) return true;
    const int k = fhp_set_kind(steady, fhp_avg_set(n));
    return k == 1 || k == 4 || k == 6;
}
template <int STEADY>  // 0 generic; 1 CFR+, 2 Linear CFR, 3 vanilla CFR, 7 Discounted CFR in their steady state; 4 CFR+ with the float32 average; 5 / 6 CFR+ deferred / catch-up;
                       // fhp_steady_pair(ka, kb): CFR+ with set A under kind ka and set B under kb
struct FhpCtxT {
    static constexpr int steady = STEADY;
    // Where the own float32 columns of the first batch are requested from HBM (opponent-only prefetch). At the board start wherever phase B has no
    // run-time branches around vector-memory operations (the CFR+ steady state; strategies that are not regret-matched): three phases of cover and an
    // empty memory queue. After phase B otherwise: the pending Vanilla / Linear average update of the opponent's walk sits behind a run-time test, the
    // compiler's wait counts at the joins are conservative, and a load in flight there is waited for in the middle of phase B (measured: the
    // best-response pass 3.06 -> 2.77 ms when its walk lost those joins; the CFR+ steady passes +4 % with the requests behind the prefetch issue).
    static constexpr bool own_after_b(int src_opp) { return src_opp == PRL_SRC_REGRET && !fhp_steady_plus(STEADY); }
    PRL_DEV PRL_INLINE int variant() const {
        if constexpr (fhp_steady_plus(STEADY)) return PRL_CFR_PLUS;
        else if constexpr (STEADY == 2) return PRL_CFR_LINEAR;
        else if constexpr (STEADY == 3) return PRL_CFR_VANILLA;
        else if constexpr (STEADY == 7) return PRL_CFR_DISCOUNTED;
        else return variant_;
    }
    PRL_DEV PRL_INLINE bool first_iteration() const { if constexpr (STEADY != 0) return false; else return iter == 0; }
    // per decision node (its set decides): how its average columns are updated by this pass
    template <int NODE>
    PRL_DEV PRL_INLINE int avg_mode() const {
        constexpr int set = fhp_avg_set(NODE);
        if constexpr (STEADY == 0) return (set == 0 ? prm->avg_pair : prm->avg_pair_b) == PRL_FHP_AVG_DEFERRED ? 0 : prm->avg_mode;
        else return fhp_may_load_avg(STEADY, NODE) ? 2 : 0;
    }
    // the blend first applies the previous iteration's step, which that iteration left out (avg_mode() == 2 whenever this holds)
    template <int NODE>
    PRL_DEV PRL_INLINE bool avg_catch_up() const {
        constexpr int set = fhp_avg_set(NODE);
        if constexpr (STEADY == 0) return (set == 0 ? prm->avg_pair : prm->avg_pair_b) == PRL_FHP_AVG_CATCH_UP;
        else return fhp_set_kind(STEADY, set) == 6;
    }
    PRL_DEV PRL_INLINE int avgsum_mask() const { if constexpr (fhp_steady_plus(STEADY)) return 0; else return prm->avgsum_mask; }
    // the running average is stored as float32 (opt-in): STEADY 4 = the CFR+ steady state with it; the generic instantiation asks at run time
    PRL_DEV PRL_INLINE bool avg32() const { if constexpr (STEADY == 4) return true; else if constexpr (STEADY != 0) return false; else return prm->avg32 != nullptr; }
    FhpLds L;
    int wave;               // workgroup's wave index, in a scalar register
    uint32_t pf_lds;        // LDS address of the prefetch area (its first segment), scalar
    uint32_t rec0, rec1;    // this lane's record of the per-card scans (phase C), read at board start
    // The lane's two positions are p0 and p0 + 1 (p0 = 2 * tid): every access of the hand-local phases at its own position is a
    // linear 8-byte LDS access, UNCONDITIONAL (an access under a lane predicate costs an exec-mask save / branch / restore). The only
    // position that is not a live hand among the walking lanes is NLIVE itself (odd count): it carries reach 0, reads the always-zero slot.
    int p0;                 // first position of this lane
    int gsm1[FHP_SLOTS];    // tie-group start - 1 (P_incl index of P[gs]), NPAD-1 (reads 0) for gs == 0 or past the live positions
    int gem1[FHP_SLOTS];    // tie-group end - 1
    bool live[FHP_SLOTS];   // the position holds a live hand (p < NLIVE)
    int c1[FHP_SLOTS], c2[FHP_SLOTS];
    int sh[FHP_SLOTS];      // hand at the position (positions NLIVE .. R-1: the hands the board blocks) -- root reach in, root vectors out
    bool active;            // p0 < NLIVE: the hand-local phases run under it (541 lanes: waves 0 .. 8)
    bool valid;             // p0 < R: the lane adds its positions' root values to the block sums (663 lanes)
    float eq_const;
    int variant_, iter;
    const PrlFhpParams* prm;
    size_t cofs;            // element offset of the lane's first position in column 0 of this board (sorted storage): + col * FHP_NP
    // the NEXT board's reach at the chance node for the lane's two positions (both seats), requested from the trunk's reach rows as soon as the
    // next board's plan has landed in the prefetch area (after the first batch's scans): chance_reach[sh] is a dependent gather from global
    // memory that used to open every board, on the critical path of phase B
    FhpF nr0, nr1;
    float nw;               // ... and that board's chance weight (chance_prob, or chance_prob x multiplicity of a weighted board): wave-uniform
    double av_old[PrlFhpShape::N_COLS][FHP_SLOTS];  // old averages in flight (fhp_request_old_average; only the updating seat's columns exist)
    bool fast;              // wave-uniform: every regret this wave holds for the board is inside the per-value box (prl_fhp_div.inc)
#ifdef PRL_FHP_TIMING
    long long t_prev, t_acc[6];
#endif
};

// ---------------------------------------------------------------------------------------------------------------------
// strategy sources (prl_fhp.h: PRL_SRC_*)
// ---------------------------------------------------------------------------------------------------------------------
// sources whose [14][R] float32 block of a board (regrets, or an explicit float32 strategy in the same layout) comes through the
// LDS prefetch area
constexpr bool fhp_src_f32_block(int src) { return src == PRL_SRC_REGRET || src == PRL_SRC_STRAT32; }
constexpr bool fhp_src_in_lds(int src) { return FHP_RG_IN_LDS && fhp_src_f32_block(src); }
template <int SRC> struct FhpScalar { typedef float type; };
template <> struct FhpScalar<PRL_SRC_UNIFORM64> { typedef double type; };
template <> struct FhpScalar<PRL_SRC_ARR64> { typedef double type; };
template <> struct FhpScalar<PRL_SRC_AVGF32> { typedef double type; };

PRL_DEV PRL_INLINE float fhp_mul_reach(float s, float r) { return s * r; }
PRL_DEV PRL_INLINE float fhp_mul_reach(double s, float r) { return (float)(s * (double)r); }

// per-board register file of one lane: raw regrets (or explicit strategy values) of all 14 action columns
struct FhpRegs {
    float rg[PrlFhpShape::N_COLS][FHP_SLOTS];    // SRC_REGRET
    double sa[PrlFhpShape::N_COLS][FHP_SLOTS];   // SRC_ARR64 / SRC_ARR32
};

template <int SRC, int A, class S, class C>
PRL_DEV PRL_INLINE void fhp_node_strategy(const C& c, const FhpRegs& R, int col0, S (&s)[3][FHP_SLOTS]) {
    if constexpr (SRC == PRL_SRC_REGRET) {
        float t[3][FHP_SLOTS], sum[FHP_SLOTS], q[3][FHP_SLOTS];
        for (int k = 0; k < FHP_SLOTS; ++k) {
            for (int i = 0; i < A; ++i) {
                float r = R.rg[col0 + i][k];
                t[i][k] = c.variant() == PRL_CFR_PLUS ? r : (r > 0.f ? r : 0.f);
            }
            sum[k] = 0.f;
            for (int i = 0; i < A; ++i) sum[k] = sum[k] + t[i][k];  // NumPy order for n < 8 (Appendix A)
        }
        fhp_regret_match<A>(t, sum, q, c.fast);
        for (int i = 0; i < A; ++i)
            for (int k = 0; k < FHP_SLOTS; ++k) s[i][k] = (S)q[i][k];
        return;
    }
    for (int k = 0; k < FHP_SLOTS; ++k) {
        if (SRC == PRL_SRC_UNIFORM64) {
            for (int i = 0; i < A; ++i) s[i][k] = (S)(1.0 / (double)A);
        } else if (SRC == PRL_SRC_STRAT32) {
            for (int i = 0; i < A; ++i) s[i][k] = (S)R.rg[col0 + i][k];
        } else if (SRC == PRL_SRC_ARR64 || SRC == PRL_SRC_AVGF32) {
            for (int i = 0; i < A; ++i) s[i][k] = (S)R.sa[col0 + i][k];
        } else {
            for (int i = 0; i < A; ++i) s[i][k] = (S)(float)R.sa[col0 + i][k];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// phase B: reach of seat Q at every terminal, compile-time DFS (StrategyFiller.py:118-146 restricted to one seat)
// ---------------------------------------------------------------------------------------------------------------------
// avg_sum of the seat whose pending average update rides on this walk, fetched before the walk starts
struct FhpAvgPre { float v[PrlFhpShape::N_COLS][FHP_SLOTS]; };

template <int Q, int S0, int S1, int NODE>
struct FhpDown {
    template <class C>
    static PRL_DEV PRL_INLINE void run(C& c, const FhpRegs& R, const FhpAvgPre& AP, const FhpV& rq, FhpF& yv) {
        constexpr int kind = PrlFhpShape::kind(NODE);
        if constexpr (kind != PRL_NODE_DECISION) {
            // the lane's two positions of this terminal's vector into the gather array: the first vector of a pair waits in `yv` for the second,
            // then one 16-byte store writes both positions of both
            constexpr int u = fhp_yord(PrlFhpShape::term_slot(NODE)), ub = fhp_y_base(u);
            if constexpr (fhp_y_step(u) == 1) fhp_lds_store2(c.L.y + ub, c.p0, rq.v);
            else if constexpr ((u & 1) == 0) yv = rq.v;
            else {
                FhpQ q;
                q[0] = yv[0]; q[1] = rq.v[0]; q[2] = yv[1]; q[3] = rq.v[1];
                *(FhpQ*)(c.L.y + (u >> 1) * (2 * FHP_NPAD) + 2 * c.p0) = q;
            }
        } else {
            constexpr int a = PrlFhpShape::actor(NODE);
            constexpr int A = PrlFhpShape::nch(NODE);
            if constexpr (a == Q) {
                constexpr int SRC = Q == 0 ? S0 : S1;
                constexpr int col0_q = PrlFhpShape::col0(NODE);  // (bound at compile time: see fhp_for_cols)
                typedef typename FhpScalar<SRC>::type S;
                S s[3][FHP_SLOTS];
                fhp_node_strategy<SRC, A, S>(c, R, col0_q, s);
                // Vanilla / Linear CFR: seat Q's pending average update (this walk has Q's new strategy AND new reach):
                // avg_sum += strategy * reach [* (iteration + 1)] (float32). The old sums were fetched before the walk
                // (fhp_seat) so that no node waits for HBM; the normalised average avg = avg_sum / sum(avg_sum) is NOT
                // written here: it is a pure function of avg_sum and is materialised when somebody reads it
                // (prl_k_fhp_avg_from_sum), which takes a float64 store stream and 14 divisions per lane out of every pass.
                if (SRC == PRL_SRC_REGRET && (c.avgsum_mask() & (1 << Q))) {
                    constexpr int col0 = PrlFhpShape::col0(NODE);
                    const int it = c.prm->avgsum_iter[Q];
                    for (int i = 0; i < A; ++i) {
                        float as[FHP_SLOTS];
                        for (int k = 0; k < FHP_SLOTS; ++k) {
                            float contrib = (float)s[i][k] * rq.v[k];
                            if (c.variant() == PRL_CFR_LINEAR) contrib = contrib * (float)(it + 1);
                            if (c.variant() == PRL_CFR_DISCOUNTED) as[k] = it > 0 ? (c.prm->dcfr_avg[Q] * AP.v[col0 + i][k]) + contrib : contrib;
                            else as[k] = it > 0 ? AP.v[col0 + i][k] + contrib : contrib;
                        }
                        fhp_gstore(c.prm->avg_sum + c.cofs + (size_t)(col0 + i) * FHP_NP, as);
                    }
                }
                FhpV cr;
                for (int k = 0; k < FHP_SLOTS; ++k) cr.v[k] = fhp_mul_reach(s[0][k], rq.v[k]);
                FhpDown<Q, S0, S1, PrlFhpShape::child(NODE, 0)>::run(c, R, AP, cr, yv);
                for (int k = 0; k < FHP_SLOTS; ++k) cr.v[k] = fhp_mul_reach(s[1][k], rq.v[k]);
                FhpDown<Q, S0, S1, PrlFhpShape::child(NODE, 1)>::run(c, R, AP, cr, yv);
                if constexpr (A > 2) {
                    for (int k = 0; k < FHP_SLOTS; ++k) cr.v[k] = fhp_mul_reach(s[2][k], rq.v[k]);
                    FhpDown<Q, S0, S1, PrlFhpShape::child(NODE, 2)>::run(c, R, AP, cr, yv);
                }
            } else {
                FhpDown<Q, S0, S1, PrlFhpShape::child(NODE, 0)>::run(c, R, AP, rq, yv);
                FhpDown<Q, S0, S1, PrlFhpShape::child(NODE, 1)>::run(c, R, AP, rq, yv);
                if constexpr (A > 2) FhpDown<Q, S0, S1, PrlFhpShape::child(NODE, 2)>::run(c, R, AP, rq, yv);
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// phases C + D: all cross-hand work of one seat's 9 terminal vectors (ValueFiller.py:103-158 generalised; canonical order)
// ---------------------------------------------------------------------------------------------------------------------
template <class C, class F>
PRL_DEV PRL_INLINE void fhp_scan_phases(C& c, F&& between_c_and_d) {
    const FhpLds& L = c.L;
    const int tid = (int)prl_tid(), wave = tid >> 6, lane = tid & 63, n_waves = FHP_THREADS / 64;
    // ---- C: per-card lists in the row16 order: lane (row r of wave w, lane i of the row) serves entries 3i .. 3i+2 of the list of
    // live card 4w + r. Every live hand is an entry of exactly two lists: its lower card's (LOWER flag) and its higher card's.
    // SPLIT K (round 5): the lower card's correction goes to K[0 .. NSHOW), the higher card's to K[NSHOW .. 2 NSHOW), each word written
    // once, and phase E adds the two at the lane's own position. Rounds 1-4 had one array: the lower card's correction was stored, the higher
    // card's waited in registers across the barrier and was then ADDED in LDS (15 scattered reads + 15 scattered writes per lane, no float
    // atomics: ~190 cycles per wave instruction on gfx950) -- 7.8 % of the best-response pass, 3 % of a CFR+ iteration, 8 % of the average-strategy
    // evaluation (profiles/r32_phaseC_knockouts.txt). The second array's 21 KB of LDS come out of the regret prefetch (below: only the
    // opponent's columns go through LDS now).
    // For a hand with tie group G (within this list: entries head .. tail), K_c = Q_excl[head] - (Q_total - Q_incl[tail]).
    // A group that crosses a lane boundary has its head in lane laneA / its tail in lane laneB of the row (precomputed in the
    // record): those lanes publish the prefix at their LAST head / FIRST tail, one cross-lane read each per vector.
    static_assert(FHP_THREADS == PRL_CLX_SLOTS * 16, "one lane per record");
    {
        float kc[3][FHP_NSHOW];
        int qpos[3];
        const uint32_t ent[3] = {c.rec0 & 0xFFFFu, c.rec0 >> 16, c.rec1 & 0xFFFFu};
        const int lane_a = (int)((c.rec1 >> 16) & 15u), lane_b = (int)((c.rec1 >> 20) & 15u), card = (int)(c.rec1 >> 24);
        const int row_base = lane & 48;
        bool head[3], tail[3], lower[3], ok[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            qpos[k] = (int)(ent[k] & 0x7FFu);
            head[k] = (ent[k] & PRL_CLX_HEAD) != 0;
            tail[k] = (ent[k] & PRL_CLX_TAIL) != 0;
            lower[k] = (ent[k] & PRL_CLX_LOWER) != 0;
            ok[k] = (ent[k] & PRL_CLX_VALID) != 0;
        }
        // the gathers are unconditional (entries past the end of a list read the always-zero slot) and independent: one 8-byte read per
        // pair of vectors and entry (12 + 3 instead of 27 for nine vectors)
        float l[3][FHP_NVEC];
#pragma unroll
        for (int j = 0; j < FHP_NPAIRS; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const FhpF t = *(const FhpF*)(L.y + j * (2 * FHP_NPAD) + 2 * qpos[k]);
                l[k][2 * j] = t[0];
                l[k][2 * j + 1] = t[1];
            }
        if constexpr (FHP_NVEC % 2 == 1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) l[k][FHP_NVEC - 1] = L.y[2 * FHP_NPAIRS * FHP_NPAD + qpos[k]];
        }
        float carry[FHP_NVEC];
#pragma unroll
        for (int v = 0; v < FHP_NVEC; ++v) {
            l[1][v] = l[0][v] + l[1][v];
            l[2][v] = l[1][v] + l[2][v];
            carry[v] = l[2][v];
        }
#pragma unroll
        for (int v = 0; v < FHP_NVEC; ++v) carry[v] = prl_row16_scan(carry[v]);  // nine independent DPP chains
#pragma unroll
        for (int v = 0; v < FHP_NVEC; ++v) carry[v] = prl_dpp_row_shr<1>(carry[v]);
        // fold vectors: only the list total Q_incl[last entry] is needed; the last entry (45) is entry 0 of lane 15
        // (l and carry are in the gather array's order: vector fhp_yord(slot) belongs to terminal `slot`)
        if ((lane & 15) == 15 && card < 64) {
            fhp_static_for<0, FHP_NFOLD>([&](auto V) __attribute__((always_inline)) {
                constexpr int v = decltype(V)::value, u = fhp_yord(FHP_NSHOW + v);
                L.Tc[v * 64 + card] = carry[u] + l[0][u];
            });
        }
        fhp_static_for<0, FHP_NSHOW>([&](auto V) __attribute__((always_inline)) {
            constexpr int v = decltype(V)::value, u = fhp_yord(v);
            const float qi0 = carry[u] + l[0][u], qi1 = carry[u] + l[1][u], qi2 = carry[u] + l[2][u];  // Q_incl of my entries
            const float qe0 = prl_dpp_row_shr<1>(qi2);                                              // Q_excl[e] = Q_incl[e - 1]
            const float tot = prl_dpp_row_share<15>(qi0);  // the list total = Q_incl of entry 45 = entry 0 of the row's lane 15
            const float out_a = head[2] ? qi1 : (head[1] ? qi0 : qe0);   // Q_excl at my last head
            const float out_b = tail[0] ? qi0 : (tail[1] ? qi1 : qi2);   // Q_incl at my first tail
            const float ra = prl_shfl(out_a, row_base + lane_a);
            const float rb = prl_shfl(out_b, row_base + lane_b);
            const float a0 = head[0] ? qe0 : ra, a1 = head[1] ? qi0 : a0, a2 = head[2] ? qi1 : a1;
            const float b2 = tail[2] ? qi2 : rb, b1 = tail[1] ? qi1 : b2, b0 = tail[0] ? qi0 : b1;
            kc[0][v] = a0 - (tot - b0);
            kc[1][v] = a1 - (tot - b1);
            kc[2][v] = a2 - (tot - b2);
        });
#pragma unroll
        for (int k = 0; k < 3; ++k) {  // unconditional: entries that do not store write a trash slot past the live positions
            const int kp = ok[k] ? qpos[k] + (lower[k] ? 0 : FHP_NSHOW * FHP_NPAD) : FHP_NPAD - 2 - (lane & 3);
#pragma unroll
            for (int v = 0; v < FHP_NSHOW; ++v) L.K[v * FHP_NPAD + kp] = kc[k][v];
        }
    }
    FHP_SYNC(c, 2);  // every gather of the terminal vectors is done: phase D overwrites the showdown vectors in place
    FHP_TICK(c, 2);
    between_c_and_d();
    // ---- D: range prefix, one wave per vector, in place: y[j] <- P[j + 1] (showdown); totals for all -------------------
    // all 17 chunks of the vector are loaded and scanned independently; only the carry adds form a chain
    // Every 5-card board leaves C(47,2) = 1081 live hands: chunks 0..15 are full (no masks, unconditional stores); chunk 16 holds 57
    // live positions, then the unused, trash and always-zero slots, which stay as they are.
    constexpr int NCH = FHP_NPAD / 64, LAST = NCH - 1, LAST_LANES = FHP_NLIVE - 64 * LAST;
    static_assert(LAST_LANES > 0 && LAST_LANES <= 64 - 7, "the last chunk ends with the unused / trash / zero slots");
    // (the stride of the vector in its array is a template argument: as a run-time value every one of the 17 chunk addresses took a register)
    auto range_prefix = [&](auto ST, const int v) __attribute__((always_inline)) {
        constexpr int st = decltype(ST)::value;
        float* y = L.y + (st == 2 ? (v >> 1) * (2 * FHP_NPAD) + (v & 1) : 2 * FHP_NPAIRS * FHP_NPAD) + st * lane;
        float incl[NCH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) incl[k] = y[st * 64 * k];
        incl[LAST] = lane < LAST_LANES ? incl[LAST] : 0.f;
        prl_wave_scan_canonical_n(incl);
        float carry = 0.f;
        constexpr unsigned SHOW = fhp_show_mask();
        const bool show = ((SHOW >> v) & 1u) != 0u;  // (v counts in the gather array's order; wave-uniform)
        if (show) {
#pragma unroll
            for (int k = 0; k < LAST; ++k) {
                y[st * 64 * k] = carry + incl[k];  // canonical P[j + 1]
                carry = carry + prl_readlane(incl[k], 63);
            }
        } else {
#pragma unroll
            for (int k = 0; k < LAST; ++k) carry = carry + prl_readlane(incl[k], 63);
        }
        const float pj = carry + incl[LAST];
        if (show && lane < LAST_LANES) y[st * 64 * LAST] = pj;
        if (lane == LAST_LANES - 1) L.Tt[v] = pj;  // (Tt in the gather array's order too)
    };
    for (int v = wave; v < FHP_NVEC; v += n_waves) {
        if (v < 2 * FHP_NPAIRS) range_prefix(std::integral_constant<int, 2>(), v);
        else range_prefix(std::integral_constant<int, 1>(), v);
    }
    prl_dma_wait();  // the next board's prefetch was issued two phases ago: landed, and visible to all after this barrier
    FHP_SYNC(c, 3);
}

// ---------------------------------------------------------------------------------------------------------------------
// order in which phase E asks HBM for the updating seat's old float64 averages (CFR+ blend). A decision node consumes its columns
// when it COMPLETES (post-order); requesting them when the walk ENTERS the node leaves the deepest nodes -- two terminals below
// them -- with ~700 cycles of cover for an HBM round trip. Pipelined order: the first two nodes of seat P in completion order are
// requested when the walk starts, and the completion of the r-th requests the (r+2)-th: every request has at least four terminal
// evaluations of cover, and at most two nodes' columns are in flight (the same peak as before, when the root's columns were in
// flight for the whole walk). The ranks count the nodes that load an average under the pass's kind (fhp_may_load_avg: with split pairs a set
// that is deferred takes no part, and the pipeline runs over the other set's nodes alone).
// ---------------------------------------------------------------------------------------------------------------------
constexpr bool fhp_is_dec_of(int P, int n) { return PrlFhpShape::kind(n) == PRL_NODE_DECISION && PrlFhpShape::actor(n) == P; }
constexpr bool fhp_completes_before(int a, int b) {  // DFS pre-order numbering: a's subtree is [a, a + size(a))
    if (a > b) return a < b + PrlFhpShape::subtree_size(b);   // a inside b's subtree
    return !(b < a + PrlFhpShape::subtree_size(a));            // a before b and b not inside a's subtree
}
constexpr int fhp_completion_rank(int steady, int P, int n) {
    int r = 0;
    for (int m = 0; m < PrlFhpShape::N_NODES; ++m)
        if (m != n && fhp_is_dec_of(P, m) && fhp_may_load_avg(steady, m) && fhp_completes_before(m, n)) ++r;
    return r;
}
constexpr int fhp_node_of_rank(int steady, int P, int r) {
    for (int m = 0; m < PrlFhpShape::N_NODES; ++m)
        if (fhp_is_dec_of(P, m) && fhp_may_load_avg(steady, m) && fhp_completion_rank(steady, P, m) == r) return m;
    return -1;
}
template <int NODE, class C>
PRL_DEV PRL_INLINE void fhp_request_old_average(C& c) {
    if constexpr (NODE >= 0) {
        constexpr int col0 = PrlFhpShape::col0(NODE);
        if (c.template avg_mode<NODE>() == 2)
#pragma unroll
        for (int i = 0; i < PrlFhpShape::nch(NODE); ++i)
        {
            if (c.avg32()) {
                float f[FHP_SLOTS];
                fhp_gload_nt(c.prm->avg32 + c.cofs + (size_t)(col0 + i) * FHP_NP, f);
                for (int k = 0; k < FHP_SLOTS; ++k) c.av_old[col0 + i][k] = (double)f[k];
            } else fhp_gload_nt(c.prm->avg + c.cofs + (size_t)(col0 + i) * FHP_NP, c.av_old[col0 + i]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// phase E: seat P's values bottom-up (ValueFiller.py:34-62 terminal scaling, :64-93 combination), regrets if updating
// ---------------------------------------------------------------------------------------------------------------------
// TC (terminal cache, UPDATE1_EVAL1): the terminal values of seat P depend on the opponent's reach only, so the second walk of that
// pass (the value of the NEW strategy) would recompute exactly what the first one computed. TC = 1: the first walk leaves each
// value where only this lane's hand reads -- K[slot][own position] (showdown) / y[slot][own position] (fold), both dead for this
// hand once read; blocked hands write their 0 into the zero slot. TC = 2: the second walk reads them back: one gather per
// terminal and slot instead of three plus the arithmetic.
template <int MODE, int P, int S0, int S1, int NODE, int TC = 0>
struct FhpUp {
    template <class C>
    static PRL_DEV PRL_INLINE void run(C& c, FhpRegs& R, FhpV& ev, FhpV& br) {
        constexpr int kind = PrlFhpShape::kind(NODE);
        const FhpLds& L = c.L;
        if constexpr (kind != PRL_NODE_DECISION) {
            constexpr int slot = PrlFhpShape::term_slot(NODE);
            // the lane's own two positions of this terminal's vector: K (planar) for a showdown, the gather array for a fold
            constexpr int yu = fhp_yord(slot), yb = fhp_y_base(yu), ys = fhp_y_step(yu);
            if constexpr (TC == 2) {
                FhpF ek;
                if constexpr (kind == PRL_NODE_TERM_SHOWDOWN) ek = fhp_lds_load2(L.K + slot * FHP_NPAD, c.p0);
                else { ek[0] = L.y[yb + ys * c.p0]; ek[1] = L.y[yb + ys * (c.p0 + 1)]; }
                ev.v = ek;
                br.v = ek;
                return;
            }
            const float pot = c.prm->pot[NODE];
            const float T = L.Tt[yu];
            FhpF e;
            if constexpr (kind == PRL_NODE_TERM_SHOWDOWN) {
                const float* Pm = L.y + yb;  // Pm[ys * j] = P[j + 1]
                FhpF p_gs, p_ge;
                for (int k = 0; k < FHP_SLOTS; ++k) {
                    p_gs[k] = Pm[ys * c.gsm1[k]];  // (the position past the live ones reads the zero slot and is masked below)
                    p_ge[k] = Pm[ys * c.gem1[k]];
                }
                const FhpF kk = fhp_lds_load2(L.K + slot * FHP_NPAD, c.p0) + fhp_lds_load2(L.K + (FHP_NSHOW + slot) * FHP_NPAD, c.p0);  // K_c1 + K_c2
                const FhpF G = p_gs - (T - p_ge);
                e = G - kk;
            } else {
                const float* Tc = L.Tc + (slot - FHP_NSHOW) * 64;
                FhpF t1, t2;
                for (int k = 0; k < FHP_SLOTS; ++k) {
                    t1[k] = Tc[c.c1[k]];
                    t2[k] = Tc[c.c2[k]];
                }
                FhpF yv;
                if constexpr (ys == 2) {  // both positions of both vectors of the pair in one 16-byte read
                    const FhpQ q = *(const FhpQ*)(L.y + (yb & ~1) + 2 * c.p0);
                    yv[0] = q[yb & 1]; yv[1] = q[2 + (yb & 1)];
                } else { yv[0] = L.y[yb + ys * c.p0]; yv[1] = L.y[yb + ys * (c.p0 + 1)]; }
                const FhpF m = t1 + t2;
                e = T - (m - yv);
            }
            e = e * c.eq_const;
            constexpr bool p_folded = kind == PRL_NODE_TERM_FOLD && PrlFhpShape::folder(NODE) == P;
            if constexpr (p_folded) e = -e;
            e = (e * pot) * 0.5f;  // (e * pot) / 2: halving is exact
            for (int k = 0; k < FHP_SLOTS; ++k) {
                const float ek = c.live[k] ? e[k] : 0.f;
                ev.v[k] = ek;
                br.v[k] = ek;
            }
            if constexpr (TC == 1) {
                if constexpr (kind == PRL_NODE_TERM_SHOWDOWN) fhp_lds_store2(L.K + slot * FHP_NPAD, c.p0, ev.v);
                else { L.y[yb + ys * c.p0] = ev.v[0]; L.y[yb + ys * (c.p0 + 1)] = ev.v[1]; }
            }
        } else {
            constexpr int a = PrlFhpShape::actor(NODE);
            constexpr int A = PrlFhpShape::nch(NODE);
            constexpr int col0 = PrlFhpShape::col0(NODE);
            constexpr bool UPD = a == P && prl_fhp_updates(MODE, P);
            if constexpr (UPD) {
                // old request order (kept for the run-time toggle): when the walk enters the node
                if (!FHP_AVG_PIPELINED(c)) fhp_request_old_average<NODE>(c);
            }
            FhpV ce[3], cb[3];
            FhpUp<MODE, P, S0, S1, PrlFhpShape::child(NODE, 0), TC>::run(c, R, ce[0], cb[0]);
            FhpUp<MODE, P, S0, S1, PrlFhpShape::child(NODE, 1), TC>::run(c, R, ce[1], cb[1]);
            if constexpr (A > 2) FhpUp<MODE, P, S0, S1, PrlFhpShape::child(NODE, 2), TC>::run(c, R, ce[2], cb[2]);
            if constexpr (a == P) {
                constexpr int SRC = P == 0 ? S0 : S1;
                typedef typename FhpScalar<SRC>::type S;
                S s[3][FHP_SLOTS];
                fhp_node_strategy<SRC, A, S>(c, R, col0, s);
                if constexpr (sizeof(S) == sizeof(float)) {  // float32 strategies: packed multiply / add over the lane's slots
                    FhpF sv[3];
                    for (int i = 0; i < A; ++i)
                        for (int k = 0; k < FHP_SLOTS; ++k) sv[i][k] = (float)s[i][k];
                    FhpF acc = sv[0] * ce[0].v;
                    for (int i = 1; i < A; ++i) acc = acc + sv[i] * ce[i].v;
                    ev.v = acc;
                } else {
                    for (int k = 0; k < FHP_SLOTS; ++k) {
                        S acc = s[0][k] * (S)ce[0].v[k];
                        for (int i = 1; i < A; ++i) acc = acc + s[i][k] * (S)ce[i].v[k];
                        ev.v[k] = (float)acc;
                    }
                }
                for (int k = 0; k < FHP_SLOTS; ++k) {
                    float mx = cb[0].v[k];
                    for (int i = 1; i < A; ++i) mx = cb[i].v[k] > mx ? cb[i].v[k] : mx;
                    br.v[k] = mx;
                }
                // regrets of the updating seat (_CFRBase.py:146-185 + CFRPlus.py:37-41 / VanillaCFR.py:26-30 / LinearCFR.py:27-31)
                if constexpr (UPD) {
                    float rn[3][FHP_SLOTS];
                    for (int i = 0; i < A; ++i) {
                        const FhpF d = ce[i].v - ev.v;
                        FhpF rv = d;
                        if (!c.first_iteration()) {
                            FhpF old;
                            for (int k = 0; k < FHP_SLOTS; ++k) old[k] = SRC == PRL_SRC_REGRET ? R.rg[col0 + i][k] : 0.f;  // untouched regrets are 0
                            if (c.variant() == PRL_CFR_DISCOUNTED) {  // old regrets discounted by sign (prl_dcfr_factors)
                                FhpF w;
                                for (int k = 0; k < FHP_SLOTS; ++k) w[k] = old[k] > 0.f ? c.prm->dcfr_pos : c.prm->dcfr_neg;
                                rv = d + (w * old);
                            } else rv = c.variant() == PRL_CFR_LINEAR ? ((float)(c.iter + 1) * d) + old : d + old;
                        }
                        for (int k = 0; k < FHP_SLOTS; ++k) {
                            float r = rv[k];
                            if (c.variant() == PRL_CFR_PLUS) r = r > 0.f ? r : 0.f;
                            rn[i][k] = r;
                        }
                        fhp_gstore_nt(c.prm->regret + c.cofs + (size_t)(col0 + i) * FHP_NP, rn[i]);
                    }
                    // the node's NEW strategy (regret matching of the regrets just written): the CFR+ average takes it
                    // (CFRPlus.py:43-87: avg = m_old * avg + m_new * strategy, float64), and UPDATE1_EVAL1's second phase E
                    // plays it -- the register file switches from regrets to strategies for this node's columns
                    constexpr bool KEEP = MODE == PRL_FHP_UPDATE1_EVAL1;
                    const int avg_mode = c.template avg_mode<NODE>();
                    if (KEEP || avg_mode) {
                        float t[3][FHP_SLOTS], sum[FHP_SLOTS];
                        for (int k = 0; k < FHP_SLOTS; ++k) {
                            sum[k] = 0.f;
                            for (int i = 0; i < A; ++i) {
                                t[i][k] = c.variant() == PRL_CFR_PLUS ? rn[i][k] : (rn[i][k] > 0.f ? rn[i][k] : 0.f);
                                sum[k] = sum[k] + t[i][k];
                            }
                        }
                        float qn[3][FHP_SLOTS];
                        // the new regrets are not covered by the board's box: per-node box (FHP_NEWSTRAT_GENERIC: plain divisions)
#if !defined(FHP_DIV_FAST) || defined(FHP_NEWSTRAT_GENERIC)
                        fhp_regret_match<A>(t, sum, qn, false);
#else
                        fhp_regret_match<A>(t, sum, qn, prl_ballot(!fhp_node_in_box<A>(t, sum)) == 0ull);
#endif
                        for (int i = 0; i < A; ++i) {
                            double an[FHP_SLOTS];
                            for (int k = 0; k < FHP_SLOTS; ++k) {
                                const float sn = qn[i][k];
                                if (KEEP) R.rg[col0 + i][k] = sn;
                                double ao = c.av_old[col0 + i][k];
                                if constexpr (SRC == PRL_SRC_REGRET) {  // (the step iteration t - 1 deferred: its strategy is the one this node just played)
                                    if (c.template avg_catch_up<NODE>()) ao = c.prm->m_old_prev * ao + c.prm->m_new_prev * (double)s[i][k];
                                }
                                an[k] = avg_mode == 2 ? c.prm->m_old * ao + c.prm->m_new * (double)sn : (double)sn;
                            }
                            if (avg_mode) {
                                if (c.avg32()) {
                                    float af[FHP_SLOTS];
                                    for (int k = 0; k < FHP_SLOTS; ++k) af[k] = (float)an[k];
                                    fhp_gstore_nt(c.prm->avg32 + c.cofs + (size_t)(col0 + i) * FHP_NP, af);
                                } else fhp_gstore_nt(c.prm->avg + c.cofs + (size_t)(col0 + i) * FHP_NP, an);
                            }
                        }
                    }
                    if constexpr (fhp_may_load_avg(C::steady, NODE)) {
                        if (FHP_AVG_PIPELINED(c)) fhp_request_old_average<fhp_node_of_rank(C::steady, P, fhp_completion_rank(C::steady, P, NODE) + 2)>(c);
                    }
                }
            } else {
                FhpF acc = ce[0].v, accb = cb[0].v;
                for (int i = 1; i < A; ++i) { acc = acc + ce[i].v; accb = accb + cb[i].v; }
                ev.v = acc;
                br.v = accb;
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// prefetch of board b into the LDS prefetch area: regrets (contiguous [14][R] block of the board), card lists, tie-group
// starts, hand-domain plan fields. Whole rows of 64 lanes x 16 bytes per DMA instruction, rows dealt round-robin to the waves.
// ---------------------------------------------------------------------------------------------------------------------
// sources of board b
struct FhpSrc { const float* rg; const uint32_t* clx; const int16_t* pp; };
PRL_DEV PRL_INLINE FhpSrc fhp_sources(const PrlFhpParams& prm, int b) {
    FhpSrc s;
    s.rg = prm.regret + (size_t)b * PrlFhpShape::N_COLS * FHP_NP;
    s.clx = prm.plan_clx + (size_t)b * PRL_CLX_WORDS;
    s.pp = prm.plan_pp + (size_t)b * PRL_PP_STRIDE;
    return s;
}

// one segment: ROWS rows of 64 x 16 bytes, dealt round-robin to the waves starting with wave START (compile time), so that
// consecutive segments keep the waves evenly loaded. Straight-line code: full rounds are unconditional, the last round is under a
// wave-uniform test (the earlier version -- a run-time chunk loop under lane predicates, with the round-robin start computed per
// segment -- cost ~330 instructions per wave and board, 15 % of the pass; this one ~120).
template <int ROWS, int START>
PRL_DEV PRL_INLINE void fhp_prefetch_segment(const void* g, uint32_t lds_addr, int wave, uint32_t lane_off) {
    constexpr int n_waves = FHP_THREADS / 64;
    const int lead = fhp_lead(g);
    int r = wave - START;
    if (r < 0) r += n_waves;
    const char* gw = (const char*)g - 4 * lead + r * 1024;  // this wave's first row (16-byte aligned); later rows at compile-time offsets
    const uint32_t lw = lds_addr + (uint32_t)r * 1024u;
#pragma unroll
    for (int i = 0; i * n_waves < ROWS; ++i)
        if ((i + 1) * n_waves <= ROWS || r + i * n_waves < ROWS) prl_lds_dma_x4_a(gw + i * n_waves * 1024, lane_off, lw + (uint32_t)(i * n_waves * 1024));
}

template <bool RG, int SEAT, class C>  // SEAT: whose regret columns (RG: if any) -- the seat whose reach the board's first batch walks
PRL_DEV PRL_INLINE void fhp_prefetch(const C& c, int b) {
    const PrlFhpParams& prm = *c.prm;
    constexpr int n_waves = FHP_THREADS / 64;
    const uint32_t lane_off = ((uint32_t)prl_tid() & 63u) * 16u;
    const int wave = c.wave;  // wave-uniform (scalar register)
    const FhpSrc src = fhp_sources(prm, b);
    constexpr int R_RG = RG ? fhp_seat_rows(SEAT) : 0, R_CLX = FHP_PF_ROWS(PRL_CLX_WORDS), R_PP = FHP_PF_ROWS(FHP_PP_WORDS);
    // LDS addresses of the areas: the area base (one scalar) + compile-time byte offsets
    const uint32_t a0 = c.pf_lds;
    constexpr uint32_t O_CLX = (FHP_RG_IN_LDS ? FHP_PF_RG_WORDS : 0) * 4u, O_PP = O_CLX + FHP_PF_AREA(PRL_CLX_WORDS) * 4u;
    if constexpr (RG) {
        fhp_static_for<0, fhp_n_runs(SEAT)>([&](auto Rn) __attribute__((always_inline)) {
            constexpr int r = decltype(Rn)::value, rows = fhp_run_rows(SEAT, r), row0 = fhp_run_row0(SEAT, r), col0 = fhp_run_col0(SEAT, r);
            fhp_prefetch_segment<rows, row0 % n_waves>(src.rg + (size_t)col0 * FHP_NP, a0 + (uint32_t)row0 * 1024u, wave, lane_off);
        });
    }
    fhp_prefetch_segment<R_CLX, R_RG % n_waves>(src.clx, a0 + O_CLX, wave, lane_off);
    fhp_prefetch_segment<R_PP, (R_RG + R_CLX) % n_waves>(src.pp, a0 + O_PP, wave, lane_off);
}

// one seat's batch; the first batch of a board issues the prefetch of the workgroup's next board (next_b, -1 = none) once
// every wave is past the barrier that follows its reads of the prefetch area
template <int MODE, int P, int S0, int S1, bool FIRST, class C>
PRL_DEV PRL_INLINE void fhp_seat(C& c, FhpRegs& R, const FhpV& r_opp, FhpV& ev, FhpV& br, int next_b) {
    if (c.active) {  // the hand-local phases run under ONE lane predicate; the waves without live positions skip them altogether
        FhpAvgPre AP;
        if ((P == 0 ? S1 : S0) == PRL_SRC_REGRET && (c.avgsum_mask() & (1 << (1 - P))) && c.prm->avgsum_iter[1 - P] > 0) {
            fhp_for_cols<0>([&](auto J) __attribute__((always_inline)) {
                constexpr int j = decltype(J)::value;
                if constexpr (PrlFhpShape::col_actor(j) == 1 - P) fhp_gload(c.prm->avg_sum + c.cofs + (size_t)j * FHP_NP, AP.v[j]);
            });
        }
        FhpF yv;
        FhpDown<1 - P, S0, S1, 0>::run(c, R, AP, r_opp, yv);
    }
    FHP_SYNC(c, 1);
    if (FIRST && next_b >= 0) fhp_prefetch<fhp_src_in_lds(P == 0 ? S1 : S0), 1 - P>(c, next_b);  // (the first batch's opponent = the next board's too)
    if constexpr (FIRST && fhp_src_f32_block(P == 0 ? S0 : S1) && C::own_after_b(P == 0 ? S1 : S0)) {
        // seat P's own float32 columns straight from HBM: consumed in phase E, two phases of cover (opponent-only prefetch, above)
        if (c.active) {
            fhp_for_cols<0>([&](auto J) __attribute__((always_inline)) {
                constexpr int j = decltype(J)::value;
                if constexpr (PrlFhpShape::col_actor(j) == P) fhp_gload(c.prm->regret + c.cofs + (size_t)j * FHP_NP, R.rg[j]);
            });
        }
    }
    FHP_TICK(c, 1);
    fhp_scan_phases(c, [&]() {});
    if (FIRST && next_b >= 0 && c.active) {  // the next board's plan is in the prefetch area and visible (barrier at the end of the scans)
        const FhpSrc nsrc = fhp_sources(*c.prm, next_b);
        const uint32_t s2 = (c.L.pf_pp + fhp_lead(nsrc.pp))[prl_tid()];
#pragma unroll
        for (int k = 0; k < FHP_SLOTS; ++k) {
            // (the raw values: multiplied by the board's weight when the next board starts -- a product here is a use, and the compiler would
            // wait for the two loads on the spot, an L2 round trip between the scans and phase E)
            const int sh = (int)((s2 >> (16 * k)) & 0xFFFFu);
            c.nr0[k] = c.prm->chance_reach[sh];
            c.nr1[k] = c.prm->chance_reach[c.prm->R + sh];
        }
    }
    if (FIRST && next_b >= 0) c.nw = c.prm->board_w[next_b];  // (a board ahead like the reach; unconditional: a select on the loaded value would be a use -> a wait on the spot)
    FHP_TICK(c, 3);
    if (c.active) {
        if constexpr (prl_fhp_updates(MODE, P)) {
            if (FHP_AVG_PIPELINED(c)) {
                fhp_request_old_average<fhp_node_of_rank(C::steady, P, 0)>(c);
                fhp_request_old_average<fhp_node_of_rank(C::steady, P, 1)>(c);
            }
        }
        if constexpr (MODE == PRL_FHP_UPDATE1_EVAL1) {
            if (FHP_TERMINAL_CACHE(c)) FhpUp<MODE, P, S0, S1, 0, 1>::run(c, R, ev, br);
            else FhpUp<MODE, P, S0, S1, 0>::run(c, R, ev, br);
        } else {
            FhpUp<MODE, P, S0, S1, 0>::run(c, R, ev, br);
        }
    }
    FHP_TICK(c, 4);
}

// ---------------------------------------------------------------------------------------------------------------------
// the board kernel: a persistent workgroup per CU walks a contiguous range of boards, each board's whole subtree on chip
// ---------------------------------------------------------------------------------------------------------------------
template <int MODE, int S0, int S1, int STEADY>
FHP_LAUNCH_BOUNDS PRL_GLOBAL void prl_k_fhp_pass(PrlFhpParams prm) {
    // the seat whose reach the first (or only) batch of a board walks: its columns come through the LDS prefetch area
    constexpr int PF_SEAT = prl_fhp_runs_seat(MODE, 0) ? 1 : 0;
    constexpr bool RG = fhp_src_in_lds(PF_SEAT == 0 ? S0 : S1);
    constexpr bool OWN_AFTER_B = FhpCtxT<STEADY>::own_after_b(PF_SEAT == 0 ? S0 : S1);
    FhpCtxT<STEADY> c;
    c.L = fhp_lds();
    c.prm = &prm;
    c.eq_const = prm.eq_const;
    for (int k = 0; k < FHP_SLOTS; ++k) { c.nr0[k] = 0.f; c.nr1[k] = 0.f; }
    c.nw = 0.f;
    c.variant_ = prm.variant;
    c.iter = prm.iter;
    const int tid = (int)prl_tid();
    c.wave = prl_wave_uniform(tid >> 6);
    c.pf_lds = prl_lds_addr(c.L.pf_rg);  // the start of the prefetch area whether or not the regret segment exists
    // boards of this workgroup: ONE contiguous range, so that a workgroup streams through its own stretch of every array (its next
    // board's block follows the current one: DRAM rows and the cache lines that two boards share stay with one CU / one XCD's L2).
    // Measured against the grid-stride order (b = workgroup, workgroup + grid, ...) with the run-time toggle: -0.9 % on well-placed
    // allocations, -3 .. -6 % on badly placed ones (profiles/r02_experiments.txt).
    // (an odd range length, so that the workgroups' streams do not share their low address bits, changes nothing: +0.2 %)
    int per_wg = (prm.n_boards + (int)prl_nblocks() - 1) / (int)prl_nblocks();
    if (prm.block_sum) per_wg = (per_wg + PRL_CHANCE_BLOCK - 1) / PRL_CHANCE_BLOCK * PRL_CHANCE_BLOCK;  // whole summation blocks
    int b = (int)prl_bid() * per_wg;
    const int b_begin = b, b_end = b + per_wg < prm.n_boards ? b + per_wg : prm.n_boards, b_step = 1;
    if (b < b_end) fhp_prefetch<RG, PF_SEAT>(c, b);  // the first board's latency is the only one that is exposed
    static_assert(PRL_CLX_ZERO_POS == FHP_NPAD - 1, "entries past the end of a card list read the always-zero slot");
    if (tid < FHP_NVEC) c.L.y[fhp_y_base(tid) + fhp_y_step(tid) * (FHP_NPAD - 1)] = 0.f;  // the always-zero slot
    if (tid < FHP_NFOLD * 64) c.L.Tc[tid] = 0.f;  // totals of board cards are never written (nothing live reads them)
    static_assert(FHP_THREADS * FHP_SLOTS >= FHP_R && FHP_NLIVE < FHP_NPAD - 6, "a lane owns two adjacent positions; trash and zero slots follow the live ones");
    c.p0 = tid * FHP_SLOTS;
    c.active = c.p0 < FHP_NLIVE;
    c.valid = c.p0 < prm.R;
    constexpr int NV = prl_fhp_out_width(MODE);
    // one row of block sums (hand order) leaves the chip: every lane stores the pair of hands 2 * tid, 2 * tid + 1 of each vector
    auto flush_block = [&](int blk) __attribute__((always_inline)) {
        if (c.valid) {
            float* o = (prm.board_out + (size_t)blk * NV * prm.R) + c.p0;
#pragma unroll
            for (int v = 0; v < NV; ++v) fhp_gstore(o + (size_t)v * prm.R, fhp_lds_load2(c.L.acc + v * FHP_R, c.p0));
        }
    };
#ifdef PRL_FHP_TIMING
    for (int i = 0; i < 6; ++i) c.t_acc[i] = 0;
    c.t_prev = __builtin_readcyclecounter();
#endif
    prl_dma_wait();
    // the FIRST board's reach at the chance node, requested here (every later board's is requested while its predecessor is walked: fhp_seat), so
    // that the loop body has ONE way of getting it: with a second one behind a test inside the loop, the join of the two paths made the compiler
    // wait -- conservatively, vmcnt counts stores too on gfx9 -- for the previous board's regret / average stores at every board start
    if (b < b_end) {
        prl_sync_lds();  // the first board's plan is in the prefetch area (DMA waited for above) and visible
        if (c.active) {
            const uint32_t s2 = (c.L.pf_pp + fhp_lead(fhp_sources(prm, prl_opaque_scalar(b)).pp))[tid];
#pragma unroll
            for (int k = 0; k < FHP_SLOTS; ++k) {
                const int sh = (int)((s2 >> (16 * k)) & 0xFFFFu);
                c.nr0[k] = prm.chance_reach[sh];
                c.nr1[k] = prm.chance_reach[prm.R + sh];
            }
        }
        c.nw = prm.board_w[b];
        for (int k = 0; k < FHP_SLOTS; ++k) {  // waited for HERE, so that the loop header sees them ready on both paths
            float a = c.nr0[k], b2 = c.nr1[k];
            prl_use(a); prl_use(b2);
            c.nr0[k] = a; c.nr1[k] = b2;
        }
        prl_use(c.nw);
    }
    for (int b_iv = b; b_iv < b_end; b_iv += b_step) {
        // the board index as an opaque scalar: every address below is a fresh function of it. (As a visible induction variable the
        // compiler strength-reduces the ~40 address expressions of the pass into 64-bit scalar induction variables kept across the
        // loop -- 70 SGPR spills.)
        const int b = prl_opaque_scalar(b_iv);
        c.cofs = (size_t)b * (PrlFhpShape::N_COLS * FHP_NP) + (size_t)c.p0;
        // the previous board is done with the work area, and this board's prefetch (waited for by every wave before the
        // last phase boundary of the previous board, or just above) is visible
        FHP_SYNC(c, 0);
        // the block that the previous board closed: its sums are complete (barrier above); the next writes to `acc` come after three
        // more barriers
        if (prm.block_sum && b_iv > b_begin && b % PRL_CHANCE_BLOCK == 0) flush_block(b / PRL_CHANCE_BLOCK - 1);
        // ---- board start: everything comes from the LDS prefetch area ----------------------------------------------------
        FhpRegs R;
        FhpV r0, r1;
        const FhpSrc src = fhp_sources(prm, b);
        {
            const uint32_t* lclx = c.L.pf_clx + fhp_lead(src.clx);
            c.rec0 = lclx[2 * tid];
            c.rec1 = lclx[2 * tid + 1];
        }
        const uint32_t* lpp = c.L.pf_pp + fhp_lead(src.pp);
        if (c.valid) {
            const uint32_t s2 = lpp[tid];  // the hands at the lane's two positions (live ones in rank order, then the blocked ones)
            c.sh[0] = (int)(s2 & 0xFFFFu);
            c.sh[1] = (int)(s2 >> 16);
        }
        for (int k = 0; k < FHP_SLOTS; ++k) { r0.v[k] = 0.f; r1.v[k] = 0.f; c.live[k] = false; }
        if (c.active) {
            const uint32_t g2 = lpp[PRL_PP_OFF_GM1 / 2 + tid], e2 = lpp[PRL_PP_OFF_EM1 / 2 + tid], c2 = lpp[PRL_PP_OFF_CC / 2 + tid];
            const float* lrg = c.L.pf_rg + fhp_lead(src.rg);
#pragma unroll
            for (int k = 0; k < FHP_SLOTS; ++k) {
                const bool live = c.p0 + k < FHP_NLIVE;
                c.live[k] = live;
                c.gsm1[k] = (int)((g2 >> (16 * k)) & 0xFFFFu);
                c.gem1[k] = (int)((e2 >> (16 * k)) & 0xFFFFu);
                const uint32_t cc = (c2 >> (16 * k)) & 0xFFFFu;
                c.c1[k] = (int)(cc & 0xFFu);
                c.c2[k] = (int)(cc >> 8);
                // chance node: both seats' reach scaled by the board probability (StrategyFiller.py:137-140,159-166); the hands the
                // board blocks have no position among the live ones
                const float w = live ? c.nw : 0.f;  // chance_prob (weighted boards: x the board's multiplicity), read a board ahead
                r0.v[k] = c.nr0[k] * w;  // requested while the previous board was walked (fhp_seat; the first board's: before the loop)
                r1.v[k] = c.nr1[k] * w;
            }
            // first the requests to HBM (explicit float64 / float32-average strategies; float32 blocks: the columns that do not come through
            // the prefetch area), then the reads of the prefetch area. ORDER: the columns phase B walks (the first batch's opponent, in the
            // order of the walk) before the other seat's, which phase E consumes: loads return in order, so a wait for the walk's first node
            // then covers two columns, not all of them -- an explicit float64 strategy is 122 KB per board, ~6 us of a CU's share of HBM, and
            // the walk used to start when the LAST column had arrived.
            auto request = [&](auto J) __attribute__((always_inline)) {
                constexpr int j = decltype(J)::value;
                constexpr int sj = PrlFhpShape::col_actor(j) == 0 ? S0 : S1;
                constexpr bool from_pf = fhp_src_in_lds(sj) && PrlFhpShape::col_actor(j) == PF_SEAT;
                const size_t col = c.cofs + (size_t)j * FHP_NP;
                if constexpr (sj == PRL_SRC_ARR64 || sj == PRL_SRC_ARR32) fhp_gload(prm.strat_arr + col, R.sa[j]);  // evaluation only: straight from HBM
                if constexpr (sj == PRL_SRC_AVGF32) {
                    float f[FHP_SLOTS];
                    fhp_gload(prm.avg32 + col, f);
                    for (int k = 0; k < FHP_SLOTS; ++k) R.sa[j][k] = (double)f[k];
                }
                // float32 blocks: the first batch's opponent comes through the prefetch area (or, where that does not fit, from HBM here: phase B
                // needs it); the other seat's columns are requested here or after phase B (FhpCtxT::own_after_b)
                if constexpr (fhp_src_f32_block(sj) && !from_pf && (PrlFhpShape::col_actor(j) == PF_SEAT || !OWN_AFTER_B)) fhp_gload(prm.regret + col, R.rg[j]);
            };
            fhp_for_cols<0>([&](auto J) __attribute__((always_inline)) { if constexpr (PrlFhpShape::col_actor(decltype(J)::value) == PF_SEAT) request(J); });
            fhp_for_cols<0>([&](auto J) __attribute__((always_inline)) { if constexpr (PrlFhpShape::col_actor(decltype(J)::value) != PF_SEAT) request(J); });
            fhp_for_cols<0>([&](auto J) __attribute__((always_inline)) {
                constexpr int j = decltype(J)::value;
                constexpr int sj = PrlFhpShape::col_actor(j) == 0 ? S0 : S1;
                constexpr bool from_pf = fhp_src_in_lds(sj) && PrlFhpShape::col_actor(j) == PF_SEAT;
                if constexpr (from_pf) {
                    constexpr int r = fhp_col_run(j), word0 = fhp_run_row0(PF_SEAT, r) * 256 + (j - fhp_run_col0(PF_SEAT, r)) * FHP_NP;
                    const FhpF v = fhp_lds_load2(lrg + word0, c.p0);
#pragma unroll
                    for (int k = 0; k < FHP_SLOTS; ++k) R.rg[j][k] = v[k];
                }
            });
#if !defined(FHP_DIV_FAST)
            c.fast = false;
#else
#error "FHP_DIV_FAST (measured and rejected in round 2): its board-start box looks at every regret column, and since round 5 the own columns are requested after phase B"
            {
                FhpBox box = fhp_box_empty();
                fhp_for_cols<0>([&](auto J) __attribute__((always_inline)) {
                    constexpr int j = decltype(J)::value;
                    constexpr int sj = PrlFhpShape::col_actor(j) == 0 ? S0 : S1;
                    if constexpr (sj == PRL_SRC_REGRET)
                        for (int k = 0; k < FHP_SLOTS; ++k) {
                            const float r = R.rg[j][k];
                            fhp_box_add(box, c.variant() == PRL_CFR_PLUS ? r : (r > 0.f ? r : 0.f));
                        }
                });
                c.fast = prl_ballot(!fhp_box_ok(box)) == 0ull;
#if defined(FHP_EXPERIMENT)
                c.fast = c.fast && FHP_EXP(c, 2);  // toggle: bit 2 = shared-reciprocal divisions
#endif
#ifdef PRL_FHP_TIMING
                if (b % 64 == 0 && (tid & 63) == 0) { atomicAdd(c.prm->timing + 6, (unsigned long long)(c.fast ? 1 : 0)); atomicAdd(c.prm->timing + 7, 1ull); }
#endif
            }
#endif
        }
        FHP_TICK(c, 0);
        // An update pass of seat p only needs seat p's values: regrets(p) read child.ev[p] and node.ev[p] only
        // (_CFRBase.py:149-158), in the subtree and in the trunk alike. The other seat's batch is skipped (its root value is
        // written as 0 and never read); the evaluation pass computes both seats.
        const int next_b = b_iv + b_step < b_end ? prl_opaque_scalar(b_iv + b_step) : -1;
        FhpV ev0, ev1, br0, br1;
        for (int k = 0; k < FHP_SLOTS; ++k) { ev0.v[k] = 0.f; ev1.v[k] = 0.f; br0.v[k] = 0.f; br1.v[k] = 0.f; }
        if constexpr (!prl_fhp_runs_seat(MODE, 0)) {
            fhp_seat<MODE, 1, S0, S1, true>(c, R, r0, ev1, br1, next_b);
            if constexpr (MODE == PRL_FHP_UPDATE1_EVAL1) {
                // seat 1's regrets (and R.rg) are updated: its value and best response under the NEW strategy, same
                // terminal vectors (they depend on seat 0 only) -- one more hand-local phase E, no scans
                if (c.active) {  // br0 := value under the new strategy
                    if (FHP_TERMINAL_CACHE(c)) FhpUp<PRL_FHP_EVAL, 1, S0, PRL_SRC_STRAT32, 0, 2>::run(c, R, br0, br1);
                    else FhpUp<PRL_FHP_EVAL, 1, S0, PRL_SRC_STRAT32, 0>::run(c, R, br0, br1);
                }
            }
        } else {
            fhp_seat<MODE, 0, S0, S1, true>(c, R, r1, ev0, br0, next_b);  // seat 0's equity is against seat 1's reach
            if constexpr (prl_fhp_runs_seat(MODE, 1)) {
                FHP_SYNC(c, 4);  // the work area is reused
                fhp_seat<MODE, 1, S0, S1, false>(c, R, r0, ev1, br1, -1);  // strategies come from the regrets held in registers
            }
        }
        if (c.valid) {
            // root vectors of this board, one row of prm.board_out: the value vectors of the seats that ran, then (modes with
            // best response) their best-response vectors; UPDATE1_EVAL1: seat 1's value, its value under the new strategy,
            // its best response. prl_fhp_out_width() is the row length in units of R. A row is in HAND order: the value of position q
            // belongs to hand sh[q]; positions NLIVE .. R-1 are the hands the board blocks, whose value is 0.
            constexpr bool BOTH = prl_fhp_runs_seat(MODE, 0) && prl_fhp_runs_seat(MODE, 1);
            constexpr int SEAT = prl_fhp_runs_seat(MODE, 0) ? 0 : 1;
            FhpF row[NV];
            if constexpr (BOTH) {
                row[0] = ev0.v; row[1] = ev1.v;
                if constexpr (prl_fhp_with_br(MODE)) { row[2] = br0.v; row[3] = br1.v; }
            } else if constexpr (MODE == PRL_FHP_UPDATE1_EVAL1) {
                row[0] = ev1.v; row[1] = br0.v; row[2] = br1.v;
            } else {
                row[0] = SEAT == 0 ? ev0.v : ev1.v;
                if constexpr (prl_fhp_with_br(MODE)) row[1] = SEAT == 0 ? br0.v : br1.v;
            }
            if (prm.block_sum) {
                // level 0 of the canonical chance sum (blocks of PRL_CHANCE_BLOCK boards, running adds in board order) happens here, in
                // LDS: every hand's running sum is touched by exactly one lane per board (the one that holds its position), the
                // barriers of the next board order the boards; a workgroup's range is a whole number of blocks, one row per BLOCK leaves
                // the chip (flush_block) and the sum kernels start a level higher
                const bool first = b % PRL_CHANCE_BLOCK == 0;
#pragma unroll
                for (int k = 0; k < FHP_SLOTS; ++k) {
                    float* a = c.L.acc + c.sh[k];
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        const float x = c.live[k] ? row[v][k] : 0.f;
                        a[v * FHP_R] = first ? x : a[v * FHP_R] + x;
                    }
                }
            } else {
                float* o = prm.board_out + (size_t)b * NV * prm.R;
#pragma unroll
                for (int k = 0; k < FHP_SLOTS; ++k)
#pragma unroll
                    for (int v = 0; v < NV; ++v) o[(size_t)v * prm.R + c.sh[k]] = c.live[k] ? row[v][k] : 0.f;
            }
        }
        FHP_TICK(c, 5);
    }
    if (prm.block_sum && b_begin < b_end) {
        prl_sync_lds();
        flush_block((b_end - 1) / PRL_CHANCE_BLOCK);
    }
#ifdef PRL_FHP_TIMING
    if (tid == 0) for (int i = 0; i < 6; ++i) atomicAdd(prm.timing + i, (unsigned long long)c.t_acc[i]);
#endif
}

// ---------------------------------------------------------------------------------------------------------------------
// launcher of this configuration
// ---------------------------------------------------------------------------------------------------------------------
template <int MODE, int S0, int S1, int STEADY = 0>
static void fhp_launch_t(const PrlFhpParams& prm, int grid, void* stream) {
    PRL_LAUNCH((prl_k_fhp_pass<MODE, S0, S1, STEADY>), grid, FHP_THREADS, FHP_LDS_BYTES, stream, prm);
}

// a pair kind of split average pairs; shapes built without them (FHP_AVG_SPLIT 0) take the generic kernel, which asks for each set's kind at run time
template <int MODE, int STEADY>
static void fhp_launch_split_t(const PrlFhpParams& prm, int grid, void* stream) {
    if constexpr (FHP_AVG_SPLIT) fhp_launch_t<MODE, PRL_SRC_REGRET, PRL_SRC_REGRET, STEADY>(prm, grid, stream);
    else fhp_launch_t<MODE, PRL_SRC_REGRET, PRL_SRC_REGRET>(prm, grid, stream);
}

int launch_pass(const PrlFhpParams& prm, int mode, int src0, int src1, void* stream) {
    if (prm.n_boards <= 0) return PRL_OK;
    if (prm.R != FHP_R) return PRL_ERR_UNSUPPORTED;  // the LDS prefetch area is laid out for 1326-hand ranges
    if (((prm.avgsum_mask & 1) && src0 != PRL_SRC_REGRET) || ((prm.avgsum_mask & 2) && src1 != PRL_SRC_REGRET)) return PRL_ERR_UNSUPPORTED;  // pending averages ride on regret-matched walks only
    static_assert(FHP_NVEC <= 16 && FHP_LDS_BYTES <= 160 * 1024, "terminal vectors + prefetch area of this shape must fit the CU's LDS");
    int grid = prm.n_boards < prm.max_grid ? prm.n_boards : prm.max_grid;
    const int key = mode * 100 + src0 * 10 + src1;
    auto kind_of = [](int pair) { return pair == PRL_FHP_AVG_DEFERRED ? 5 : pair == PRL_FHP_AVG_CATCH_UP ? 6 : 1; };
    // steady-state kinds (FhpCtxT): CFR+ blending its running average, or Linear / vanilla CFR, after the first iteration
    const int steady = prm.no_steady || prm.iter == 0 ? 0
                       : (prm.variant == PRL_CFR_PLUS && prm.avg_mode == 2 && prm.avgsum_mask == 0)
                           ? (prm.avg32 ? 4 : fhp_steady_pair(kind_of(prm.avg_pair), kind_of(prm.avg_pair_b)))
                       : (prm.variant == PRL_CFR_LINEAR && prm.avg_mode == 0) ? 2
                       : (prm.variant == PRL_CFR_VANILLA && prm.avg_mode == 0) ? 3
                       : (prm.variant == PRL_CFR_DISCOUNTED && prm.avg_mode == 0) ? 7 : 0;
    switch (key) {
        case PRL_FHP_UPDATE0 * 100 + PRL_SRC_UNIFORM64 * 10 + PRL_SRC_UNIFORM64: fhp_launch_t<PRL_FHP_UPDATE0, PRL_SRC_UNIFORM64, PRL_SRC_UNIFORM64>(prm, grid, stream); break;
        case PRL_FHP_UPDATE1 * 100 + PRL_SRC_REGRET * 10 + PRL_SRC_UNIFORM64: fhp_launch_t<PRL_FHP_UPDATE1, PRL_SRC_REGRET, PRL_SRC_UNIFORM64>(prm, grid, stream); break;
        case PRL_FHP_UPDATE0 * 100 + PRL_SRC_REGRET * 10 + PRL_SRC_REGRET: fhp_launch_t<PRL_FHP_UPDATE0, PRL_SRC_REGRET, PRL_SRC_REGRET>(prm, grid, stream); break;
        case PRL_FHP_UPDATE1 * 100 + PRL_SRC_REGRET * 10 + PRL_SRC_REGRET: fhp_launch_t<PRL_FHP_UPDATE1, PRL_SRC_REGRET, PRL_SRC_REGRET>(prm, grid, stream); break;
        case PRL_FHP_UPDATE0_EVAL * 100 + PRL_SRC_REGRET * 10 + PRL_SRC_REGRET: fhp_launch_t<PRL_FHP_UPDATE0_EVAL, PRL_SRC_REGRET, PRL_SRC_REGRET>(prm, grid, stream); break;
        // the two passes of a steady-state iteration have a CFR+ specialisation (FhpCtxT); the pairs of unequal kinds are the ones the split schedule
        // of prl_solver_iterations takes: (D,U) opens a call, (C,D) / (D,C) alternate, (C,U) / (U,C) close it. Any other pair: the generic kernel
        case PRL_FHP_UPDATE0_BR * 100 + PRL_SRC_REGRET * 10 + PRL_SRC_REGRET:
            if (steady == 1) fhp_launch_t<PRL_FHP_UPDATE0_BR, PRL_SRC_REGRET, PRL_SRC_REGRET, 1>(prm, grid, stream);
            else if (steady == 4) fhp_launch_t<PRL_FHP_UPDATE0_BR, PRL_SRC_REGRET, PRL_SRC_REGRET, 4>(prm, grid, stream);
            else if (steady == 5) fhp_launch_t<PRL_FHP_UPDATE0_BR, PRL_SRC_REGRET, PRL_SRC_REGRET, 5>(prm, grid, stream);
            else if (steady == 6) fhp_launch_t<PRL_FHP_UPDATE0_BR, PRL_SRC_REGRET, PRL_SRC_REGRET, 6>(prm, grid, stream);
            else if (steady == fhp_steady_pair(5, 1)) fhp_launch_split_t<PRL_FHP_UPDATE0_BR, fhp_steady_pair(5, 1)>(prm, grid, stream);
            else if (steady == fhp_steady_pair(6, 5)) fhp_launch_split_t<PRL_FHP_UPDATE0_BR, fhp_steady_pair(6, 5)>(prm, grid, stream);
            else if (steady == fhp_steady_pair(5, 6)) fhp_launch_split_t<PRL_FHP_UPDATE0_BR, fhp_steady_pair(5, 6)>(prm, grid, stream);
            else if (steady == fhp_steady_pair(6, 1)) fhp_launch_split_t<PRL_FHP_UPDATE0_BR, fhp_steady_pair(6, 1)>(prm, grid, stream);
            else if (steady == fhp_steady_pair(1, 6)) fhp_launch_split_t<PRL_FHP_UPDATE0_BR, fhp_steady_pair(1, 6)>(prm, grid, stream);
            else if (steady == 2) fhp_launch_t<PRL_FHP_UPDATE0_BR, PRL_SRC_REGRET, PRL_SRC_REGRET, 2>(prm, grid, stream);
            else if (steady == 3) fhp_launch_t<PRL_FHP_UPDATE0_BR, PRL_SRC_REGRET, PRL_SRC_REGRET, 3>(prm, grid, stream);
            else if (steady == 7) fhp_launch_t<PRL_FHP_UPDATE0_BR, PRL_SRC_REGRET, PRL_SRC_REGRET, 7>(prm, grid, stream);
            else fhp_launch_t<PRL_FHP_UPDATE0_BR, PRL_SRC_REGRET, PRL_SRC_REGRET>(prm, grid, stream);
            break;
        case PRL_FHP_UPDATE1_EVAL1 * 100 + PRL_SRC_REGRET * 10 + PRL_SRC_REGRET:
            if (steady == 1) fhp_launch_t<PRL_FHP_UPDATE1_EVAL1, PRL_SRC_REGRET, PRL_SRC_REGRET, 1>(prm, grid, stream);
            else if (steady == 4) fhp_launch_t<PRL_FHP_UPDATE1_EVAL1, PRL_SRC_REGRET, PRL_SRC_REGRET, 4>(prm, grid, stream);
            else if (steady == 5) fhp_launch_t<PRL_FHP_UPDATE1_EVAL1, PRL_SRC_REGRET, PRL_SRC_REGRET, 5>(prm, grid, stream);
            else if (steady == 6) fhp_launch_t<PRL_FHP_UPDATE1_EVAL1, PRL_SRC_REGRET, PRL_SRC_REGRET, 6>(prm, grid, stream);
            else if (steady == fhp_steady_pair(5, 1)) fhp_launch_split_t<PRL_FHP_UPDATE1_EVAL1, fhp_steady_pair(5, 1)>(prm, grid, stream);
            else if (steady == fhp_steady_pair(6, 5)) fhp_launch_split_t<PRL_FHP_UPDATE1_EVAL1, fhp_steady_pair(6, 5)>(prm, grid, stream);
            else if (steady == fhp_steady_pair(5, 6)) fhp_launch_split_t<PRL_FHP_UPDATE1_EVAL1, fhp_steady_pair(5, 6)>(prm, grid, stream);
            else if (steady == fhp_steady_pair(6, 1)) fhp_launch_split_t<PRL_FHP_UPDATE1_EVAL1, fhp_steady_pair(6, 1)>(prm, grid, stream);
            else if (steady == fhp_steady_pair(1, 6)) fhp_launch_split_t<PRL_FHP_UPDATE1_EVAL1, fhp_steady_pair(1, 6)>(prm, grid, stream);
            else if (steady == 2) fhp_launch_t<PRL_FHP_UPDATE1_EVAL1, PRL_SRC_REGRET, PRL_SRC_REGRET, 2>(prm, grid, stream);
            else if (steady == 3) fhp_launch_t<PRL_FHP_UPDATE1_EVAL1, PRL_SRC_REGRET, PRL_SRC_REGRET, 3>(prm, grid, stream);
            else if (steady == 7) fhp_launch_t<PRL_FHP_UPDATE1_EVAL1, PRL_SRC_REGRET, PRL_SRC_REGRET, 7>(prm, grid, stream);
            else fhp_launch_t<PRL_FHP_UPDATE1_EVAL1, PRL_SRC_REGRET, PRL_SRC_REGRET>(prm, grid, stream);
            break;
        case PRL_FHP_EVAL0 * 100 + PRL_SRC_REGRET * 10 + PRL_SRC_REGRET: fhp_launch_t<PRL_FHP_EVAL0, PRL_SRC_REGRET, PRL_SRC_REGRET>(prm, grid, stream); break;
        case PRL_FHP_EVAL * 100 + PRL_SRC_UNIFORM64 * 10 + PRL_SRC_UNIFORM64: fhp_launch_t<PRL_FHP_EVAL, PRL_SRC_UNIFORM64, PRL_SRC_UNIFORM64>(prm, grid, stream); break;
        case PRL_FHP_EVAL * 100 + PRL_SRC_REGRET * 10 + PRL_SRC_REGRET: fhp_launch_t<PRL_FHP_EVAL, PRL_SRC_REGRET, PRL_SRC_REGRET>(prm, grid, stream); break;
        case PRL_FHP_EVAL * 100 + PRL_SRC_ARR64 * 10 + PRL_SRC_ARR64: fhp_launch_t<PRL_FHP_EVAL, PRL_SRC_ARR64, PRL_SRC_ARR64>(prm, grid, stream); break;
        case PRL_FHP_EVAL * 100 + PRL_SRC_STRAT32 * 10 + PRL_SRC_STRAT32: fhp_launch_t<PRL_FHP_EVAL, PRL_SRC_STRAT32, PRL_SRC_STRAT32>(prm, grid, stream); break;
        case PRL_FHP_EVAL * 100 + PRL_SRC_AVGF32 * 10 + PRL_SRC_AVGF32: fhp_launch_t<PRL_FHP_EVAL, PRL_SRC_AVGF32, PRL_SRC_AVGF32>(prm, grid, stream); break;
        case PRL_FHP_EVAL * 100 + PRL_SRC_ARR32 * 10 + PRL_SRC_ARR32: fhp_launch_t<PRL_FHP_EVAL, PRL_SRC_ARR32, PRL_SRC_ARR32>(prm, grid, stream); break;
        default: return PRL_ERR_UNSUPPORTED;
    }
    return PRL_OK;
}

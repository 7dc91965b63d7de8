// Street kernels of the per-street fused engine (prl_st.h), included once per registered spec by prl_st_kernels.hip inside a
// namespace. Expects ST_SPEC (the spec struct of prl_fhp.h), ST_THREADS (768), FHP_SLOTS (2) and ST_LAUNCH_BOUNDS.
//
//   prl_k_st_down<S0, S1>                   non-final streets: both seats' reach at every "go on" leaf, hand-local, no LDS
//   prl_k_st_pass<LAST, MODE, S0, S1, ST>   one workgroup walks one street instance at a time (persistent, contiguous range):
//       B  seat Q's reach at the terminals (and, on the last street, at the showdown leaves) into the rank-sorted domain in LDS
//       C  per-card blocker scans in the row16 order; last street: the board pass's record-driven scan of all vectors with the
//          showdown corrections K; other streets: totals only (fold terminals), lists read from the plan
//       D  range prefix (last street: in place, P[j+1]) / range totals (other streets)
//       E  seat P's values bottom-up: fold / showdown terminals from LDS, "go on" leaves = canonical chance sum of the child
//          instances' root vectors; regret / strategy / average update of the seat being updated; root vectors -> val
// Arithmetic, association orders and pass modes are those of the single-deal board pass (prl_fhp_pass.inc, DESIGN.md section 3):
// the results are bit-identical to the level-synchronous engine and to the oracle.
// Memory traffic of an instance (DESIGN.md section 4b): its record (PrlStInst) and its root's reach rows are fetched while the PREVIOUS instance
// is walked (record through an LDS double buffer, a dword per lane of wave 0); the opponent's columns when the instance starts (non-final
// streets: before anything else); the updating seat's columns while the scans run; its old averages two nodes ahead of the value walk; rows
// are addressed as (wave-uniform pointer, 32-bit lane offset that is opaque per instance): see st_at and prl_opaque_lane for why.
typedef PrlFhpDerive<ST_SPEC> StShape;
static_assert(StShape::subtree_size(0) == StShape::N_NODES, "the spec is one DFS pre-order tree");
#define ST_R 1326
#define ST_NL (StShape::N_SHOW)   // "go on" leaves (showdowns on the last street)
#define ST_NF (StShape::N_FOLD)
#define ST_NCOLS (StShape::N_COLS)
#define ST_MAXA (StShape::MAX_A)  // actions of a decision node: the first extent of every per-action array below
static_assert(ST_NF >= 1 && ST_NL >= 1, "a street subtree has fold terminals and leaves");

#include "prl_fhp_div.inc"
struct StV { FhpF v; };

template <bool LAST> constexpr int st_npad() { return LAST ? 1088 : 1216; }  // >= live hands + 7 spare slots, multiple of 64
template <bool LAST> constexpr int st_nvec() { return LAST ? ST_NL + ST_NF : ST_NF; }
constexpr int st_leaf_index(int n) { return StShape::count_kind(PRL_NODE_TERM_SHOWDOWN, n); }
template <bool LAST> constexpr int st_slot(int n) {  // slot of a terminal among the vectors in LDS (leaves first on the last street)
    return StShape::kind(n) == PRL_NODE_TERM_SHOWDOWN ? (LAST ? st_leaf_index(n) : -1)
         : StShape::kind(n) == PRL_NODE_TERM_FOLD ? (LAST ? ST_NL : 0) + StShape::count_kind(PRL_NODE_TERM_FOLD, n) : -1;
}
#define ST_NLIVE_LAST 1081  // C(47, 2)
#define ST_INST_WORDS ((int)(sizeof(PrlStInst) / 4))
#define ST_CL_ROUNDS 2  // 4 cards per wave and round, 12 waves: 52 cards in two rounds
static_assert(4 * (ST_THREADS / 64) * ST_CL_ROUNDS >= 52, "the per-card scans of a non-final street cover the deck");
static_assert(sizeof(PrlStInst) == 192 && ST_INST_WORDS <= 64, "an instance record is read by one wave, a dword per lane");
template <bool LAST> constexpr size_t st_lds_bytes() {
    return ((size_t)st_nvec<LAST>() * st_npad<LAST>() + (LAST ? (size_t)ST_NL * st_npad<LAST>() : 0) + (size_t)ST_NF * 64 + 32 + 2 * ST_INST_WORDS) * 4;
}
// any registered shape may turn up on the last street, where the showdown vectors and their corrections join the fold vectors in LDS
static_assert(st_lds_bytes<true>() <= 160 * 1024 && st_lds_bytes<false>() <= 160 * 1024, "this shape does not fit the CU's LDS on the last street: it cannot be registered");

// ---- global access helpers: a lane owns the two adjacent hands 2 tid, 2 tid + 1 (one 8 / 16-byte access) ------------------------
// address of a lane's pair in an array whose row pointer is wave-uniform: a uniform 64-bit base plus a 32-bit unsigned BYTE offset per lane, the
// form the global instructions take as (SGPR pair, VGPR offset) -- as `uniform + gofs` with a signed index every access built its own
// 64-bit per-lane pointer (67 v_lshl_add_u64 and as many VGPR pairs in the 27-node shape's update pass)
template <class T> PRL_DEV PRL_INLINE T* st_at(T* uniform_row, unsigned gofs) {
#if defined(PRL_EMU)
    return uniform_row + gofs;
#else
    typedef typename std::conditional<std::is_const<T>::value, const char, char>::type B;
    return (T*)((B*)uniform_row + (size_t)(gofs * (unsigned)sizeof(T)));
#endif
}
template <class T> struct alignas(2 * sizeof(T)) StPair { T a, b; };
template <class T> PRL_DEV PRL_INLINE void st_gload(const T* p, T (&out)[2]) { const StPair<T> v = *(const StPair<T>*)p; out[0] = v.a; out[1] = v.b; }
template <class T> PRL_DEV PRL_INLINE void st_gstore(T* p, const T (&in)[2]) { StPair<T> v; v.a = in[0]; v.b = in[1]; *(StPair<T>*)p = v; }
PRL_DEV PRL_INLINE FhpF st_gload_f(const float* p) { float t[2]; st_gload(p, t); FhpF r; r[0] = t[0]; r[1] = t[1]; return r; }
PRL_DEV PRL_INLINE void st_gstore_f(float* p, const FhpF& in) { float t[2] = {in[0], in[1]}; st_gstore(p, t); }
template <class T> PRL_DEV PRL_INLINE void st_gstore_nt(T* p, const T (&in)[2]) {
#if defined(PRL_EMU)
    st_gstore(p, in);
#else
    if constexpr (sizeof(T) == 4) { typedef float v2 __attribute__((ext_vector_type(2))); v2 v; v.x = in[0]; v.y = in[1]; __builtin_nontemporal_store(v, (v2*)p); }
    else { typedef double d2 __attribute__((ext_vector_type(2))); d2 v; v.x = in[0]; v.y = in[1]; __builtin_nontemporal_store(v, (d2*)p); }
#endif
}
PRL_DEV PRL_INLINE void st_gload_nt(const double* p, double (&out)[2]) {
#if defined(PRL_EMU)
    st_gload(p, out);
#else
    typedef double d2 __attribute__((ext_vector_type(2)));
    const d2 v = __builtin_nontemporal_load((const d2*)p);
    out[0] = v.x; out[1] = v.y;
#endif
}
PRL_DEV PRL_INLINE void st_gload_nt(const float* p, float (&out)[2]) {
#if defined(PRL_EMU)
    st_gload(p, out);
#else
    typedef float v2 __attribute__((ext_vector_type(2)));
    const v2 v = __builtin_nontemporal_load((const v2*)p);
    out[0] = v.x; out[1] = v.y;
#endif
}

// PRL_ST_TIMING builds: wave 0 of every workgroup accumulates the shader clock spent between phase boundaries (last street only)
#if defined(PRL_ST_TIMING) && !defined(PRL_EMU)
#define ST_TICK(c, i) do { if (prl_tid() == 0 && (c).prm->timing) { const long long t_ = clock64(); atomicAdd((c).prm->timing + (i), (unsigned long long)(t_ - (c).t_prev)); (c).t_prev = t_; } } while (0)
#else
#define ST_TICK(c, i) do { } while (0)
#endif

// ---- context ---------------------------------------------------------------------------------------------------------------------
template <int STEADY>  // 0 generic; 1 CFR+ (4: with the float32 running average), 2 Linear CFR, 3 vanilla CFR in their steady state (as FhpCtxT of the board pass)
struct StCtx {
    // the running average is stored as float32 (opt-in): a compile-time fact in the steady kernels -- a run-time branch around the average's loads and
    // stores gets conservative wait counts at its joins (measured: 2.50 instead of 2.37 ms per iteration with the test at run time)
    PRL_DEV PRL_INLINE bool avg32() const { if constexpr (STEADY == 4) return true; else if constexpr (STEADY != 0) return false; else return prm->avg32 != nullptr; }
    PRL_DEV PRL_INLINE int variant() const {
        if constexpr (STEADY == 1 || STEADY == 4) return PRL_CFR_PLUS;
        else if constexpr (STEADY == 2) return PRL_CFR_LINEAR;
        else if constexpr (STEADY == 3) return PRL_CFR_VANILLA;
        else return variant_;
    }
    PRL_DEV PRL_INLINE bool first_iteration() const { if constexpr (STEADY != 0) return false; else return iter == 0; }
    PRL_DEV PRL_INLINE int avg_mode() const { if constexpr (STEADY == 1 || STEADY == 4) return 2; else if constexpr (STEADY >= 2) return 0; else return prm->avg_mode; }
    PRL_DEV PRL_INLINE int avgsum_mask() const { if constexpr (STEADY == 1 || STEADY == 4) return 0; else return prm->avgsum_mask; }
    float *y, *K, *Tc, *Tt;  // LDS: terminal vectors (sorted domain), showdown corrections, per-card totals, range totals
    float* potL;             // LDS: this instance's pots per node. (Read from the instance table in HBM, every terminal of the value walk
                             // waited for a load that queues behind the walk's own stores and prefetches: vmcnt counts in order.)
    int n_kids, kid_base;    // this instance's children on the next street (uniform; read once per instance for the same reason)
    // the NEXT instance of this workgroup, fetched while this one is walked: its record (a dword per lane of wave 0, through LDS) and its
    // root's reach rows -- two dependent round trips that used to open every instance
    uint32_t* inst_next;     // LDS: the other half of the record double buffer
    uint32_t nx_word;
    bool has_next;
    float pp0[2], pp1[2];
    int wave;
    uint32_t rec0, rec1;     // last street: this lane's record of the per-card scans
    int posw[2], posz[2], gsm1[2], gem1[2];
    bool live[2];
    int c1[2], c2[2];
    bool valid;
    unsigned gofs;
    float eq_const;
    int variant_, iter;
    const PrlStParams* prm;
    size_t col_base_i;       // first internal column of this instance
    int n_live, n_t, plan;   // other streets: live hands / entries per card list / plan row of this instance
    int16_t clq[2][3];       // other streets: this lane's entries of the plan's per-card lists, per round of st_scan_inner (ST_CL_ROUNDS)
    double av_old[ST_NCOLS][2];
#if defined(PRL_ST_TIMING)
    long long t_prev;
#endif
};

struct StRegs {
    float rg[ST_NCOLS][2];    // PRL_SRC_REGRET / STRAT32
    double sa[ST_NCOLS][2];   // PRL_SRC_ARR64 / ARR32
};
struct StAvgPre { float v[ST_NCOLS][2]; };

template <int SRC> struct StScalar { typedef float type; };
template <> struct StScalar<PRL_SRC_UNIFORM64> { typedef double type; };
template <> struct StScalar<PRL_SRC_ARR64> { typedef double type; };
template <> struct StScalar<PRL_SRC_AVGF32> { typedef double type; };  // the float32 running average, widened and played with float64 arithmetic
PRL_DEV PRL_INLINE float st_mul_reach(float s, float r) { return s * r; }
PRL_DEV PRL_INLINE float st_mul_reach(double s, float r) { return (float)(s * (double)r); }
constexpr bool st_src_f32_block(int src) { return src == PRL_SRC_REGRET || src == PRL_SRC_STRAT32; }

// Everything derived from the shape must be a COMPILE-TIME constant where it is used: the derivations (PrlFhpDerive) are nested loops over
// the listing, and one that survives into the kernel runs as scalar code per instance (a `#pragma unroll` loop over the columns that
// asks col_actor(j) was measured at ~49 000 scalar instructions per instance on the 27-node shape: 17x the whole pass). Hence: loops
// over columns are template recursions (J a template parameter), and every derived value is bound to a `constexpr` local.
template <int J, int N, class F>
PRL_DEV PRL_INLINE void st_static_for(F&& f) {
    if constexpr (J < N) {
        f(std::integral_constant<int, J>());
        st_static_for<J + 1, N>(f);
    }
}

// the columns of one seat's decision nodes, straight from HBM into registers
template <int SEAT, int S0, int S1, int J, class C>
PRL_DEV PRL_INLINE void st_load_cols_from(const C& c, StRegs& R) {
    if constexpr (J < ST_NCOLS) {
        constexpr int SRC = SEAT == 0 ? S0 : S1;
        constexpr int actor = StShape::col_actor(J);
        if constexpr (actor == SEAT) {
            const size_t col = (c.col_base_i + J) * (size_t)c.prm->R;  // uniform
            if constexpr (SRC == PRL_SRC_ARR64 || SRC == PRL_SRC_ARR32) st_gload(st_at(c.prm->strat_arr + col, c.gofs), R.sa[J]);
            if constexpr (SRC == PRL_SRC_AVGF32) {
                float f[2];
                st_gload(st_at((const float*)c.prm->avg32 + col, c.gofs), f);
                R.sa[J][0] = (double)f[0]; R.sa[J][1] = (double)f[1];
            }
            if constexpr (st_src_f32_block(SRC)) st_gload(st_at((const float*)c.prm->regret + col, c.gofs), R.rg[J]);
        }
        st_load_cols_from<SEAT, S0, S1, J + 1>(c, R);
    }
}
template <int SEAT, int S0, int S1, class C>
PRL_DEV PRL_INLINE void st_load_cols(const C& c, StRegs& R) { st_load_cols_from<SEAT, S0, S1, 0>(c, R); }

// the old avg_sum values of seat SEAT's columns (Vanilla / Linear: the pending average update of the reach walk)
template <int SEAT, int J, class C>
PRL_DEV PRL_INLINE void st_load_avg_sum_from(const C& c, StAvgPre& AP) {
    if constexpr (J < ST_NCOLS) {
        constexpr int actor = StShape::col_actor(J);
        if constexpr (actor == SEAT) st_gload(st_at((const float*)c.prm->avg_sum + (c.col_base_i + J) * (size_t)c.prm->R, c.gofs), AP.v[J]);
        st_load_avg_sum_from<SEAT, J + 1>(c, AP);
    }
}

template <int SRC, int A, class S, class C>
PRL_DEV PRL_INLINE void st_node_strategy(const C& c, const StRegs& R, int col0, S (&s)[ST_MAXA][2]) {
    if constexpr (SRC == PRL_SRC_REGRET) {
        float t[ST_MAXA][2], sum[2], q[ST_MAXA][2];
        for (int k = 0; k < 2; ++k) {
            for (int i = 0; i < A; ++i) {
                const float r = R.rg[col0 + i][k];
                t[i][k] = c.variant() == PRL_CFR_PLUS ? r : (r > 0.f ? r : 0.f);
            }
            sum[k] = 0.f;
            for (int i = 0; i < A; ++i) sum[k] = sum[k] + t[i][k];  // NumPy order for n < 8 (SURVEY Appendix A)
        }
        fhp_regret_match_generic<A>(t, sum, q);
        for (int i = 0; i < A; ++i)
            for (int k = 0; k < 2; ++k) s[i][k] = (S)q[i][k];
        return;
    }
    for (int k = 0; k < 2; ++k) {
        if (SRC == PRL_SRC_UNIFORM64) { for (int i = 0; i < A; ++i) s[i][k] = (S)(1.0 / (double)A); }
        else if (SRC == PRL_SRC_STRAT32) { for (int i = 0; i < A; ++i) s[i][k] = (S)R.rg[col0 + i][k]; }
        else if (SRC == PRL_SRC_ARR64 || SRC == PRL_SRC_AVGF32) { for (int i = 0; i < A; ++i) s[i][k] = (S)R.sa[col0 + i][k]; }
        else { for (int i = 0; i < A; ++i) s[i][k] = (S)(float)R.sa[col0 + i][k]; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// DOWN: both seats' reach from the instance root to its "go on" leaves (StrategyFiller.py:118-146), hand-local
// ---------------------------------------------------------------------------------------------------------------------------------
template <int S0, int S1, int NODE>
struct StPush {
    template <class C>
    static PRL_DEV PRL_INLINE void run(const C& c, const StRegs& R, float* out, const StV& r0, const StV& r1) {
        constexpr int kind = StShape::kind(NODE);
        if constexpr (kind == PRL_NODE_TERM_SHOWDOWN) {
            constexpr int leaf = st_leaf_index(NODE);
            float* o = out + (size_t)leaf * 2 * c.prm->R;  // uniform
            st_gstore_f(st_at(o, c.gofs), r0.v);
            st_gstore_f(st_at(o + c.prm->R, c.gofs), r1.v);
        } else if constexpr (kind == PRL_NODE_DECISION) {
            constexpr int a = StShape::actor(NODE), A = StShape::nch(NODE), SRC = a == 0 ? S0 : S1, col0 = StShape::col0(NODE);
            typedef typename StScalar<SRC>::type S;
            S s[ST_MAXA][2];
            st_node_strategy<SRC, A, S>(c, R, col0, s);
            st_static_for<0, A>([&](auto ic) {
                constexpr int I = decltype(ic)::value, KID = StShape::child(NODE, I);
                StV cr;
                for (int k = 0; k < 2; ++k) cr.v[k] = st_mul_reach(s[I][k], a == 0 ? r0.v[k] : r1.v[k]);
                if constexpr (a == 0) StPush<S0, S1, KID>::run(c, R, out, cr, r1);
                else StPush<S0, S1, KID>::run(c, R, out, r0, cr);
            });
        }
    }
};

struct StDownCtx {  // the slice of StCtx the strategy helpers read
    PRL_DEV PRL_INLINE int variant() const { return variant_; }
    int variant_;
    unsigned gofs;
    size_t col_base_i;
    const PrlStParams* prm;
};

template <int S0, int S1>
ST_LAUNCH_BOUNDS PRL_GLOBAL void prl_k_st_down(PrlStParams prm) {
    const int tid = (int)prl_tid();
    const bool valid = tid * 2 < prm.R;
    StDownCtx c;
    c.prm = &prm;
    c.variant_ = prm.variant;
    c.gofs = valid ? (unsigned)tid * 2u : 0u;
    for (int i_iv = (int)prl_bid(); i_iv < prm.n_inst; i_iv += (int)prl_nblocks()) {
        const int i = prl_opaque_scalar(i_iv);
        const PrlStInst* in = prm.inst + i;
        c.col_base_i = (size_t)prm.col_base + (size_t)i * ST_NCOLS;
        if (!valid) continue;
        int16_t pos[2];
        st_gload(st_at(prm.plan_pos + (size_t)in->row * prm.plan_stride, c.gofs), pos);
        float p0[2], p1[2];
        const float* pr = prm.parent_reach + (size_t)in->parent_slot * 2 * prm.R;
        st_gload(st_at(pr, c.gofs), p0);
        st_gload(st_at(pr + prm.R, c.gofs), p1);
        StV r0, r1;
        for (int k = 0; k < 2; ++k) {
            const float w = pos[k] >= 0 ? in->w : 0.f;  // StrategyFiller.py:137-140,159-166: 0 for hands the new cards block
            r0.v[k] = p0[k] * w;
            r1.v[k] = p1[k] * w;
        }
        StRegs R;
        st_load_cols<0, S0, S1>(c, R);
        st_load_cols<1, S0, S1>(c, R);
        StPush<S0, S1, 0>::run(c, R, prm.leaf_reach + (size_t)in->leaf_slot0 * 2 * prm.R, r0, r1);  // (the street's buffer: the groups of a street share it)
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// phase B: reach of seat Q at the terminals of the instance (and its pending Vanilla / Linear average update, as the board pass)
// ---------------------------------------------------------------------------------------------------------------------------------
template <bool LAST, int Q, int S0, int S1, int NODE>
struct StDown {
    template <class C>
    static PRL_DEV PRL_INLINE void run(C& c, const StRegs& R, const StAvgPre& AP, const StV& rq) {
        constexpr int kind = StShape::kind(NODE);
        if constexpr (kind != PRL_NODE_DECISION) {
            constexpr int slot = st_slot<LAST>(NODE);
            if constexpr (slot >= 0) {
                for (int k = 0; k < 2; ++k) c.y[slot * st_npad<LAST>() + c.posw[k]] = rq.v[k];
            }
        } else {
            constexpr int a = StShape::actor(NODE), A = StShape::nch(NODE);
            if constexpr (a == Q) {
                constexpr int SRC = Q == 0 ? S0 : S1, col0 = StShape::col0(NODE);
                typedef typename StScalar<SRC>::type S;
                S s[ST_MAXA][2];
                st_node_strategy<SRC, A, S>(c, R, col0, s);
                if (c.avgsum_mask() & (1 << Q)) {  // VanillaCFR.py:40-55, LinearCFR.py:41-57: avg_sum += strategy * reach [* (t + 1)]
                    const int it = c.prm->avgsum_iter[Q];
                    for (int i = 0; i < A; ++i) {
                        float as[2];
                        for (int k = 0; k < 2; ++k) {
                            float contrib = (float)s[i][k] * rq.v[k];
                            if (c.variant() == PRL_CFR_LINEAR) contrib = contrib * (float)(it + 1);
                            if (c.variant() == PRL_CFR_DISCOUNTED) as[k] = it > 0 ? (c.prm->dcfr_avg[Q] * AP.v[col0 + i][k]) + contrib : contrib;
                            else as[k] = it > 0 ? AP.v[col0 + i][k] + contrib : contrib;
                        }
                        st_gstore(st_at(c.prm->avg_sum + (c.col_base_i + col0 + i) * (size_t)c.prm->R, c.gofs), as);
                    }
                }
                st_static_for<0, A>([&](auto ic) {
                    constexpr int I = decltype(ic)::value;
                    StV cr;
                    for (int k = 0; k < 2; ++k) cr.v[k] = st_mul_reach(s[I][k], rq.v[k]);
                    StDown<LAST, Q, S0, S1, StShape::child(NODE, I)>::run(c, R, AP, cr);
                });
            } else {
                st_static_for<0, A>([&](auto ic) { StDown<LAST, Q, S0, S1, StShape::child(NODE, decltype(ic)::value)>::run(c, R, AP, rq); });
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------------------------
// phases C + D
// ---------------------------------------------------------------------------------------------------------------------------------
// last street: the board pass's scan phases (prl_fhp_pass.inc: fhp_scan_phases) for this shape's vectors
template <class C, class F>
PRL_DEV PRL_INLINE void st_scan_last(C& c, F&& between_c_and_d) {
    constexpr int NPAD = st_npad<true>(), NVEC = st_nvec<true>(), NSHOW = ST_NL, NFOLD = ST_NF;
    const int tid = (int)prl_tid(), wave = tid >> 6, lane = tid & 63, n_waves = ST_THREADS / 64;
    static_assert(ST_THREADS == PRL_CLX_SLOTS * 16, "one lane per record");
    float kc[3][NSHOW];
    int qpos[3];
    bool hi_add[3];
    {
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
            hi_add[k] = ok[k] && !lower[k];
        }
        float l[3][NVEC];
#pragma unroll
        for (int v = 0; v < NVEC; ++v)
#pragma unroll
            for (int k = 0; k < 3; ++k) l[k][v] = c.y[v * NPAD + qpos[k]];
        float carry[NVEC];
#pragma unroll
        for (int v = 0; v < NVEC; ++v) {
            l[1][v] = l[0][v] + l[1][v];
            l[2][v] = l[1][v] + l[2][v];
            carry[v] = l[2][v];
        }
#pragma unroll
        for (int v = 0; v < NVEC; ++v) carry[v] = prl_row16_scan(carry[v]);
#pragma unroll
        for (int v = 0; v < NVEC; ++v) carry[v] = prl_dpp_row_shr<1>(carry[v]);
        if ((lane & 15) == 15 && card < 64) {  // fold vectors: the list total = Q_incl[last entry] (entry 0 of lane 15 on a 5-card board)
#pragma unroll
            for (int v = 0; v < NFOLD; ++v) c.Tc[v * 64 + card] = carry[NSHOW + v] + l[0][NSHOW + v];
        }
#pragma unroll
        for (int v = 0; v < NSHOW; ++v) {
            const float qi0 = carry[v] + l[0][v], qi1 = carry[v] + l[1][v], qi2 = carry[v] + l[2][v];
            const float qe0 = prl_dpp_row_shr<1>(qi2);
            const float tot = prl_shfl(qi0, row_base + 15);
            const float out_a = head[2] ? qi1 : (head[1] ? qi0 : qe0);
            const float out_b = tail[0] ? qi0 : (tail[1] ? qi1 : qi2);
            const float ra = prl_shfl(out_a, row_base + lane_a);
            const float rb = prl_shfl(out_b, row_base + lane_b);
            const float a0 = head[0] ? qe0 : ra, a1 = head[1] ? qi0 : a0, a2 = head[2] ? qi1 : a1;
            const float b2 = tail[2] ? qi2 : rb, b1 = tail[1] ? qi1 : b2, b0 = tail[0] ? qi0 : b1;
            kc[0][v] = a0 - (tot - b0);
            kc[1][v] = a1 - (tot - b1);
            kc[2][v] = a2 - (tot - b2);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int kp = (ok[k] && lower[k]) ? qpos[k] : NPAD - 2 - (lane & 3);
#pragma unroll
            for (int v = 0; v < NSHOW; ++v) c.K[v * NPAD + kp] = kc[k][v];
        }
    }
    prl_sync_lds();
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (hi_add[k]) {
#pragma unroll
            for (int v = 0; v < NSHOW; ++v) c.K[v * NPAD + qpos[k]] = c.K[v * NPAD + qpos[k]] + kc[k][v];
        }
    between_c_and_d();
    constexpr int NCH = NPAD / 64, LASTC = NCH - 1, LAST_LANES = ST_NLIVE_LAST - 64 * LASTC;
    static_assert(LAST_LANES > 0 && LAST_LANES <= 64 - 7, "the last chunk ends with the unused / trash / zero slots");
    for (int v = wave; v < NVEC; v += n_waves) {
        float* y = c.y + v * NPAD;
        float incl[NCH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) incl[k] = y[64 * k + lane];
        incl[LASTC] = lane < LAST_LANES ? incl[LASTC] : 0.f;
        prl_wave_scan_canonical_n(incl);
        float carry = 0.f;
        if (v < NSHOW) {
#pragma unroll
            for (int k = 0; k < LASTC; ++k) {
                y[64 * k + lane] = carry + incl[k];  // canonical P[j + 1]
                carry = carry + prl_readlane(incl[k], 63);
            }
        } else {
#pragma unroll
            for (int k = 0; k < LASTC; ++k) carry = carry + prl_readlane(incl[k], 63);
        }
        const float pj = carry + incl[LASTC];
        if (v < NSHOW && lane < LAST_LANES) y[64 * LASTC + lane] = pj;
        if (lane == LAST_LANES - 1) c.Tt[v] = pj;
    }
    prl_sync_lds();
}

// other streets: only fold terminals. Per-card totals Q_c[n_t] in the row16 order (4 cards per wave at a time, lists from the plan)
// and the range total P[n] (chunked wave scans, sequential carries) of every fold vector.
template <class C, class F>
PRL_DEV PRL_INLINE void st_scan_inner(C& c, F&& between_c_and_d) {
    constexpr int NPAD = st_npad<false>(), NFOLD = ST_NF;
    const int tid = (int)prl_tid(), wave = tid >> 6, lane = tid & 63, n_waves = ST_THREADS / 64, row = lane >> 4, l16 = lane & 15;
    const int n_cards = c.prm->n_cards;
#pragma unroll
    for (int rd = 0; rd < ST_CL_ROUNDS; ++rd) {
        const int c0 = 4 * (wave + rd * n_waves);
        if (c0 >= n_cards) break;  // wave-uniform
        const int card = c0 + row;
        const bool okc = card < n_cards;
        int qpos[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int q = (int)c.clq[rd][k];  // (requested with the plan fields: -1 past the end of the list / for a card that does not exist)
            qpos[k] = q >= 0 ? q : NPAD - 1;  // the always-zero slot
        }
        float l[3][NFOLD];
#pragma unroll
        for (int v = 0; v < NFOLD; ++v)
#pragma unroll
            for (int k = 0; k < 3; ++k) l[k][v] = c.y[v * NPAD + qpos[k]];
        float carry[NFOLD];
#pragma unroll
        for (int v = 0; v < NFOLD; ++v) {
            l[1][v] = l[0][v] + l[1][v];
            l[2][v] = l[1][v] + l[2][v];
            carry[v] = l[2][v];
        }
#pragma unroll
        for (int v = 0; v < NFOLD; ++v) carry[v] = prl_row16_scan(carry[v]);
#pragma unroll
        for (int v = 0; v < NFOLD; ++v) carry[v] = prl_dpp_row_shr<1>(carry[v]);
        if (l16 == 15 && okc) {  // Q_incl[n_t - 1] = carry of lane 15 + its local prefix (entries past the end add 0)
#pragma unroll
            for (int v = 0; v < NFOLD; ++v) c.Tc[v * 64 + card] = carry[v] + l[2][v];
        }
    }
    between_c_and_d();
    const int n = c.n_live, n_ch = (n + 63) >> 6;
    for (int v = wave; v < NFOLD; v += n_waves) {
        const float* y = c.y + v * NPAD;
        float carry = 0.f;
        for (int k = 0; k < n_ch; ++k) {
            const int j = 64 * k + lane;
            float x = j < n ? y[j] : 0.f;
            x = prl_wave_scan_canonical(x);
            if (k < n_ch - 1) carry = carry + prl_readlane(x, 63);
            else if (lane == ((n - 1) & 63)) c.Tt[v] = carry + x;
        }
    }
    prl_sync_lds();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// phase E
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr bool st_is_dec_of(int P, int n) { return StShape::kind(n) == PRL_NODE_DECISION && StShape::actor(n) == P; }
constexpr bool st_completes_before(int a, int b) {
    if (a > b) return a < b + StShape::subtree_size(b);
    return !(b < a + StShape::subtree_size(a));
}
constexpr int st_completion_rank(int P, int n) {
    int r = 0;
    for (int m = 0; m < StShape::N_NODES; ++m)
        if (m != n && st_is_dec_of(P, m) && st_completes_before(m, n)) ++r;
    return r;
}
constexpr int st_node_of_rank(int P, int r) {
    for (int m = 0; m < StShape::N_NODES; ++m)
        if (st_is_dec_of(P, m) && st_completion_rank(P, m) == r) return m;
    return -1;
}
template <int NODE, class C>
PRL_DEV PRL_INLINE void st_request_old_average(C& c) {
    if constexpr (NODE >= 0) {
        constexpr int col0 = StShape::col0(NODE), A = StShape::nch(NODE);
#pragma unroll
        for (int i = 0; i < A; ++i) {
            const size_t col = (c.col_base_i + col0 + i) * (size_t)c.prm->R;
            if (c.avg32()) {  // float32 storage: read, widened; the blend below is float64 as ever
                float f[2];
                st_gload_nt(st_at((const float*)c.prm->avg32 + col, c.gofs), f);
                c.av_old[col0 + i][0] = (double)f[0]; c.av_old[col0 + i][1] = (double)f[1];
            } else st_gload_nt(st_at((const double*)c.prm->avg + col, c.gofs), c.av_old[col0 + i]);
        }
    }
}

// value of "go on" leaf `leaf`: the canonical chance sum (ValueFiller.py:76-78; running adds nested as blocks of 32 outcomes, groups of
// 32 blocks, then the groups -- prl_chance_sum of the level-synchronous engine) over the child instances' root vectors, component comp
// The rows of ST_LEAF_BATCH children are requested together and added in order: the adds form the canonical chain either way, but a load per
// add (the straightforward loop) exposes one memory round trip per child (measured on the non-final streets: ~0.8 us each, 36 per instance
// with two outcomes per deal). Children past the end of a block re-read its last row and are not added.
#define ST_LEAF_BATCH 4
template <bool TWO, class C>
PRL_DEV PRL_INLINE void st_leaf_sum2(const C& c, int leaf, int comp_a, int comp_b, FhpF& out_a, FhpF& out_b) {
    const PrlStParams& prm = *c.prm;
    const int nk = c.n_kids;
    const size_t row = (size_t)prm.child_w * prm.R, stride = (size_t)ST_NL * row;  // outcome k + 1 of the same leaf is ST_NL instances on
    const float* pa = prm.child_val + ((size_t)c.kid_base + leaf) * row + (size_t)comp_a * prm.R;  // uniform; the lane's offset is added per access
    const float* pb = prm.child_val + ((size_t)c.kid_base + leaf) * row + (size_t)comp_b * prm.R;
    FhpF total_a = FhpF{}, total_b = FhpF{};
    for (int g0 = 0, gi = 0; g0 < nk; g0 += PRL_CHANCE_BLOCK * PRL_CHANCE_BLOCK, ++gi) {
        const int g1 = g0 + PRL_CHANCE_BLOCK * PRL_CHANCE_BLOCK < nk ? g0 + PRL_CHANCE_BLOCK * PRL_CHANCE_BLOCK : nk;
        FhpF gsum_a = FhpF{}, gsum_b = FhpF{};
        for (int b0 = g0, bi = 0; b0 < g1; b0 += PRL_CHANCE_BLOCK, ++bi) {
            const int b1 = b0 + PRL_CHANCE_BLOCK < g1 ? b0 + PRL_CHANCE_BLOCK : g1;
            FhpF bsum_a = FhpF{}, bsum_b = FhpF{};
            for (int i0 = b0; i0 < b1; i0 += ST_LEAF_BATCH) {
                FhpF ta[ST_LEAF_BATCH], tb[ST_LEAF_BATCH];
#pragma unroll
                for (int j = 0; j < ST_LEAF_BATCH; ++j) {
                    const int i = i0 + j < b1 ? i0 + j : b1 - 1;  // uniform
                    ta[j] = st_gload_f(st_at(pa + (size_t)i * stride, c.gofs));
                    if constexpr (TWO) tb[j] = st_gload_f(st_at(pb + (size_t)i * stride, c.gofs));
                }
#pragma unroll
                for (int j = 0; j < ST_LEAF_BATCH; ++j) {
                    if (i0 + j < b1) {
                        bsum_a = i0 + j == b0 ? ta[j] : bsum_a + ta[j];
                        if constexpr (TWO) bsum_b = i0 + j == b0 ? tb[j] : bsum_b + tb[j];
                    }
                }
            }
            gsum_a = bi == 0 ? bsum_a : gsum_a + bsum_a;
            if constexpr (TWO) gsum_b = bi == 0 ? bsum_b : gsum_b + bsum_b;
        }
        total_a = gi == 0 ? gsum_a : total_a + gsum_a;
        if constexpr (TWO) total_b = gi == 0 ? gsum_b : total_b + gsum_b;
    }
    out_a = total_a;
    if constexpr (TWO) out_b = total_b;
}
// components of a child row (prl_fhp_out_width): where seat P's value / best response sit. WALK2: the second walk of UPDATE1_EVAL1
template <int MODE, int P, bool WALK2> constexpr int st_comp_ev() {
    constexpr bool both = prl_fhp_runs_seat(MODE, 0) && prl_fhp_runs_seat(MODE, 1);
    return WALK2 ? 1 : both ? P : 0;
}
template <int MODE, int P, bool WALK2> constexpr int st_comp_br() {  // -1: the mode carries no best response for this walk
    constexpr bool both = prl_fhp_runs_seat(MODE, 0) && prl_fhp_runs_seat(MODE, 1);
    return WALK2 ? 2 : MODE == PRL_FHP_UPDATE1_EVAL1 ? -1 : !prl_fhp_with_br(MODE) ? -1 : both ? 2 + P : 1;
}

// TC: terminal cache of UPDATE1_EVAL1 (1: the first walk leaves every terminal value at the hand's own position, 2: the second walk
// reads it back). ROWMODE: the pass's mode (what the child rows hold); MODE: what this walk does (EVAL for the second walk).
template <bool LAST, int ROWMODE, int MODE, int P, int S0, int S1, int NODE, int TC = 0>
struct StUp {
    template <class C>
    static PRL_DEV PRL_INLINE void run(C& c, StRegs& R, StV& ev, StV& br) {
        constexpr int kind = StShape::kind(NODE);
        constexpr int NPAD = st_npad<LAST>();
        if constexpr (kind == PRL_NODE_TERM_SHOWDOWN && !LAST) {
            constexpr int leaf = st_leaf_index(NODE);
            constexpr int ce = st_comp_ev<ROWMODE, P, TC == 2>(), cb = st_comp_br<ROWMODE, P, TC == 2>();
            // (requesting all leaves' sums ahead of the walk, while the scans run, was measured: no gain, 36-54 more live registers)
            if constexpr (cb >= 0) st_leaf_sum2<true>(c, leaf, ce, cb, ev.v, br.v);
            else { st_leaf_sum2<false>(c, leaf, ce, ce, ev.v, br.v); br.v = ev.v; }
        } else if constexpr (kind != PRL_NODE_DECISION) {
            constexpr int slot = st_slot<LAST>(NODE);
            float* cache = kind == PRL_NODE_TERM_SHOWDOWN ? c.K + slot * NPAD : c.y + slot * NPAD;
            if constexpr (TC == 2) {
                for (int k = 0; k < 2; ++k) {
                    const float ek = cache[c.posz[k]];
                    ev.v[k] = ek;
                    br.v[k] = ek;
                }
                return;
            }
            const float pot = c.potL[NODE];
            const float T = c.Tt[slot];
            FhpF e;
            if constexpr (kind == PRL_NODE_TERM_SHOWDOWN) {
                const float* Pm = c.y + slot * NPAD;  // Pm[j] = P[j + 1]
                FhpF p_gs, p_ge, kk;
                for (int k = 0; k < 2; ++k) {
                    p_gs[k] = Pm[c.gsm1[k]];
                    p_ge[k] = Pm[c.gem1[k]];
                    kk[k] = c.K[slot * NPAD + c.posz[k]];
                }
                const FhpF G = p_gs - (T - p_ge);
                e = G - kk;
            } else {
                const float* Tc = c.Tc + (slot - (LAST ? ST_NL : 0)) * 64;
                FhpF t1, t2, yv;
                for (int k = 0; k < 2; ++k) {
                    t1[k] = Tc[prl_opaque_lane(c.c1[k])];  // (opaque: the address is computed here, not before the instance loop)
                    t2[k] = Tc[prl_opaque_lane(c.c2[k])];
                    yv[k] = c.y[slot * NPAD + c.posz[k]];
                }
                const FhpF m = t1 + t2;
                e = T - (m - yv);
            }
            e = e * c.eq_const;
            constexpr bool p_folded = kind == PRL_NODE_TERM_FOLD && StShape::folder(NODE) == P;
            if constexpr (p_folded) e = -e;
            e = (e * pot) * 0.5f;  // (e * pot) / 2: halving is exact
            for (int k = 0; k < 2; ++k) {
                const float ek = c.live[k] ? e[k] : 0.f;
                ev.v[k] = ek;
                br.v[k] = ek;
                if constexpr (TC == 1) cache[c.posz[k]] = ek;
            }
        } else {
            constexpr int a = StShape::actor(NODE), A = StShape::nch(NODE), col0 = StShape::col0(NODE);
            constexpr bool UPD = a == P && prl_fhp_updates(MODE, P);
            StV ce[ST_MAXA], cb[ST_MAXA];
            st_static_for<0, A>([&](auto ic) {
                constexpr int I = decltype(ic)::value;
                StUp<LAST, ROWMODE, MODE, P, S0, S1, StShape::child(NODE, I), TC>::run(c, R, ce[I], cb[I]);
            });
            if constexpr (a == P) {
                constexpr int SRC = P == 0 ? S0 : S1;
                typedef typename StScalar<SRC>::type S;
                S s[ST_MAXA][2];
                st_node_strategy<SRC, A, S>(c, R, col0, s);
                if constexpr (sizeof(S) == sizeof(float)) {
                    FhpF sv[ST_MAXA];
                    for (int i = 0; i < A; ++i)
                        for (int k = 0; k < 2; ++k) sv[i][k] = (float)s[i][k];
                    FhpF acc = sv[0] * ce[0].v;
                    for (int i = 1; i < A; ++i) acc = acc + sv[i] * ce[i].v;
                    ev.v = acc;
                } else {
                    for (int k = 0; k < 2; ++k) {
                        S acc = s[0][k] * (S)ce[0].v[k];
                        for (int i = 1; i < A; ++i) acc = acc + s[i][k] * (S)ce[i].v[k];
                        ev.v[k] = (float)acc;
                    }
                }
                for (int k = 0; k < 2; ++k) {
                    float mx = cb[0].v[k];
                    for (int i = 1; i < A; ++i) mx = cb[i].v[k] > mx ? cb[i].v[k] : mx;
                    br.v[k] = mx;
                }
                if constexpr (UPD) {  // _CFRBase.py:146-185 + CFRPlus.py:37-41 / VanillaCFR.py:26-30 / LinearCFR.py:27-31
                    float rn[ST_MAXA][2];
                    for (int i = 0; i < A; ++i) {
                        const FhpF d = ce[i].v - ev.v;
                        FhpF rv = d;
                        if (!c.first_iteration()) {
                            FhpF old;
                            for (int k = 0; k < 2; ++k) old[k] = SRC == PRL_SRC_REGRET ? R.rg[col0 + i][k] : 0.f;
                            if (c.variant() == PRL_CFR_DISCOUNTED) {  // old regrets discounted by sign (prl_dcfr_factors)
                                FhpF w;
                                for (int k = 0; k < 2; ++k) w[k] = old[k] > 0.f ? c.prm->dcfr_pos : c.prm->dcfr_neg;
                                rv = d + (w * old);
                            } else rv = c.variant() == PRL_CFR_LINEAR ? ((float)(c.iter + 1) * d) + old : d + old;
                        }
                        for (int k = 0; k < 2; ++k) {
                            float r = rv[k];
                            if (c.variant() == PRL_CFR_PLUS) r = r > 0.f ? r : 0.f;
                            rn[i][k] = r;
                        }
                        st_gstore_nt(st_at(c.prm->regret + (c.col_base_i + col0 + i) * (size_t)c.prm->R, c.gofs), rn[i]);
                    }
                    constexpr bool KEEP = MODE == PRL_FHP_UPDATE1_EVAL1;
                    if (KEEP || c.avg_mode()) {
                        float t[ST_MAXA][2], sum[2];
                        for (int k = 0; k < 2; ++k) {
                            sum[k] = 0.f;
                            for (int i = 0; i < A; ++i) {
                                t[i][k] = c.variant() == PRL_CFR_PLUS ? rn[i][k] : (rn[i][k] > 0.f ? rn[i][k] : 0.f);
                                sum[k] = sum[k] + t[i][k];
                            }
                        }
                        float qn[ST_MAXA][2];
                        fhp_regret_match_generic<A>(t, sum, qn);
                        for (int i = 0; i < A; ++i) {
                            double an[2];
                            for (int k = 0; k < 2; ++k) {
                                const float sn = qn[i][k];
                                if (KEEP) R.rg[col0 + i][k] = sn;
                                an[k] = c.avg_mode() == 2 ? c.prm->m_old * c.av_old[col0 + i][k] + c.prm->m_new * (double)sn : (double)sn;
                            }
                            if (c.avg_mode()) {
                                const size_t col = (c.col_base_i + col0 + i) * (size_t)c.prm->R;
                                if (c.avg32()) {  // rounded on the store: a <- float32(m_old * a + m_new * s)
                                    float af[2] = {(float)an[0], (float)an[1]};
                                    st_gstore_nt(st_at(c.prm->avg32 + col, c.gofs), af);
                                } else st_gstore_nt(st_at(c.prm->avg + col, c.gofs), an);
                            }
                        }
                    }
                    if (c.avg_mode() == 2) st_request_old_average<st_node_of_rank(P, st_completion_rank(P, NODE) + 2)>(c);
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

// one seat's batch. FIRST: the first batch of the instance loads the columns it needs (Q's before the reach walk, P's while the scans
// run); a second batch (modes that run both seats) finds both seats' columns in registers. Requesting Q's columns earlier -- at the end
// of the previous instance, or at the top of the loop before the table entry is read -- was measured 14-20 % SLOWER on the 27-node shape
// (profiles/r05_experiments.txt): the 26 registers live across the instance boundary cost more than the exposed round trip.
template <bool LAST, int MODE, int P, int S0, int S1, bool FIRST, class C>
PRL_DEV PRL_INLINE void st_seat(C& c, StRegs& R, const StV& r_opp, StV& ev, StV& br) {
    if (c.valid) {
        if constexpr (FIRST && LAST) st_load_cols<1 - P, S0, S1>(c, R);  // (other streets: requested at the top of the instance, below)
        StAvgPre AP;
        if ((c.avgsum_mask() & (1 << (1 - P))) && c.prm->avgsum_iter[1 - P] > 0) st_load_avg_sum_from<1 - P, 0>(c, AP);
        StDown<LAST, 1 - P, S0, S1, 0>::run(c, R, AP, r_opp);
    }
    ST_TICK(c, 1);  // opponent columns + reach walk
    if constexpr (FIRST) {
        if (c.has_next && prl_tid() < ST_INST_WORDS) c.inst_next[prl_tid()] = c.nx_word;  // requested when this instance started
    }
    prl_sync_lds();
    ST_TICK(c, 2);  // barrier wait
    if constexpr (FIRST) {
        if (c.has_next && c.valid) {
            const int parent = prl_wave_uniform((int)c.inst_next[1]);
            const float* pr = c.prm->parent_reach + (size_t)parent * 2 * c.prm->R;
            st_gload(st_at(pr, c.gofs), c.pp0);
            st_gload(st_at(pr + c.prm->R, c.gofs), c.pp1);
        }
    }
    auto fetch_p = [&]() {  // seat P's columns are requested while the scans run
        if (c.valid) {
            if constexpr (FIRST) st_load_cols<P, S0, S1>(c, R);
        }
    };
    if constexpr (LAST) st_scan_last(c, fetch_p);
    else st_scan_inner(c, fetch_p);
    ST_TICK(c, 3);  // scans C + D with their barriers
    if (c.valid) {
        // the first old averages: requested here, not with the columns -- across phase D the compiler has no registers for them, waited for
        // each request and spilled it (three exposed round trips per instance in the ISA of the 27-node shape)
        if constexpr (prl_fhp_updates(MODE, P)) {
            if (c.avg_mode() == 2) {
                st_request_old_average<st_node_of_rank(P, 0)>(c);
                st_request_old_average<st_node_of_rank(P, 1)>(c);
            }
        }
        if constexpr (MODE == PRL_FHP_UPDATE1_EVAL1) StUp<LAST, MODE, MODE, P, S0, S1, 0, 1>::run(c, R, ev, br);
        else StUp<LAST, MODE, MODE, P, S0, S1, 0>::run(c, R, ev, br);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the pass kernel: a persistent workgroup per CU walks a contiguous range of instances
// ---------------------------------------------------------------------------------------------------------------------------------
template <bool LAST, int MODE, int S0, int S1, int STEADY>
ST_LAUNCH_BOUNDS PRL_GLOBAL void prl_k_st_pass(PrlStParams prm) {
    constexpr int NPAD = st_npad<LAST>(), NVEC = st_nvec<LAST>();
    StCtx<STEADY> c;
    {
        float* f = (float*)prl_smem();
        c.y = f; f += NVEC * NPAD;
        c.K = f; f += LAST ? ST_NL * NPAD : 0;
        c.Tc = f; f += ST_NF * 64;
        c.Tt = f; f += 32;
        c.inst_next = (uint32_t*)f;  // [2][ST_INST_WORDS]: set per instance below
    }
    uint32_t* const inst_buf = c.inst_next;
    c.prm = &prm;
    c.eq_const = prm.eq_const;
    c.variant_ = prm.variant;
    c.iter = prm.iter;
    const int tid = (int)prl_tid();
    c.wave = prl_wave_uniform(tid >> 6);
    const int per_wg = (prm.n_inst + (int)prl_nblocks() - 1) / (int)prl_nblocks();
    const int i_begin = (int)prl_bid() * per_wg;
    const int i_end = i_begin + per_wg < prm.n_inst ? i_begin + per_wg : prm.n_inst;
    if (tid < NVEC) c.y[tid * NPAD + NPAD - 1] = 0.f;             // the always-zero slot
    if (LAST && tid < ST_NL) c.K[tid * NPAD + NPAD - 1] = 0.f;
    if (tid < ST_NF * 64) c.Tc[tid] = 0.f;                        // totals of board cards are never written (only blocked hands read them)
    c.valid = tid * 2 < prm.R;
    const unsigned gofs0 = c.valid ? (unsigned)tid * 2u : 0u;
    c.gofs = gofs0;
    {
        uint16_t cc[2];
        st_gload(st_at(prm.hole_packed, c.gofs), cc);
        for (int k = 0; k < 2; ++k) { c.c1[k] = (int)(cc[k] & 0xFFu); c.c2[k] = (int)(cc[k] >> 8); }
    }
#if defined(PRL_ST_TIMING)
    c.t_prev = clock64();
#endif
    int plan_loaded = -1;
    // the first instance's record and root reach: the only exposed fetch of these (every later instance finds them prefetched)
    if (i_begin < i_end) {
        const PrlStInst* in0 = prm.inst + i_begin;
        if (tid < ST_INST_WORDS) inst_buf[tid] = ((const uint32_t*)in0)[tid];
        for (int k = 0; k < 2; ++k) { c.pp0[k] = 0.f; c.pp1[k] = 0.f; }
        if (c.valid) {
            const float* pr = prm.parent_reach + (size_t)in0->parent_slot * 2 * prm.R;
            st_gload(st_at(pr, c.gofs), c.pp0);
            st_gload(st_at(pr + prm.R, c.gofs), c.pp1);
        }
    }
    for (int i_iv = i_begin; i_iv < i_end; ++i_iv) {
        const int i = prl_opaque_scalar(i_iv);
        c.gofs = (unsigned)prl_opaque_lane((int)gofs0);  // (not loop-invariant to the optimiser: see st_at)
        c.col_base_i = (size_t)prm.col_base + (size_t)i * ST_NCOLS;
        const int half = (i_iv - i_begin) & 1;
        const uint32_t* rec = inst_buf + half * ST_INST_WORDS;  // this instance's record (PrlStInst as dwords)
        c.inst_next = inst_buf + (half ^ 1) * ST_INST_WORDS;
        c.potL = (float*)(rec + 8);
        c.has_next = i_iv + 1 < i_end;
        c.nx_word = 0u;
        if (c.has_next && tid < ST_INST_WORDS) c.nx_word = ((const uint32_t*)(prm.inst + i + 1))[tid];
        StRegs R;
        if constexpr (!LAST) {
            // the opponent's columns of the first batch before anything else: these kernels walk one or two instances per workgroup with the
            // whole latency of every request exposed, and have the registers to spare (the last street's pass does not: -14 % when tried)
            constexpr int P_FIRST = prl_fhp_runs_seat(MODE, 0) ? 0 : 1;
            if (c.valid) st_load_cols<1 - P_FIRST, S0, S1>(c, R);
        }
        ST_TICK(c, 5);   // row stores, loop turn-around
        prl_sync_lds();  // the previous instance is done with the work area; this instance's record is in LDS
        ST_TICK(c, 6);   // barrier wait
        const int plan = prl_wave_uniform((int)rec[0]);
        const float inst_w = __builtin_bit_cast(float, (uint32_t)prl_wave_uniform((int)rec[2]));
        c.n_kids = prl_wave_uniform((int)rec[3]);
        c.kid_base = prl_wave_uniform((int)rec[4]);
        const int val_slot = prl_wave_uniform((int)rec[5]);  // its row in the street's buffer (where its parent looks for it)
        if (plan != plan_loaded) {  // adjacent instances share their board: the lane's plan fields stay in registers
            plan_loaded = plan;
            c.plan = plan;
            if constexpr (LAST) {
                const uint32_t* clx = prm.plan_clx + (size_t)plan * PRL_CLX_WORDS;
                c.rec0 = clx[2 * tid];
                c.rec1 = clx[2 * tid + 1];
            } else {
                c.n_live = prm.plan_nlive[plan];
                c.n_t = prm.n_cards - 1 - prm.plan_ndealt[plan];
                // this lane's entries of the per-card lists (st_scan_inner: rounds of 4 cards per wave), requested with the plan fields
                const int16_t* cl = prm.plan_cl + (size_t)plan * prm.cl_stride;
                const int row = (tid & 63) >> 4, l16 = tid & 15, n_waves = ST_THREADS / 64;
#pragma unroll
                for (int rd = 0; rd < ST_CL_ROUNDS; ++rd) {
                    const int card = 4 * (c.wave + rd * n_waves) + row;
                    const bool okc = card < prm.n_cards;
                    const int16_t* lst = cl + (size_t)(okc ? card : 0) * (prm.n_cards - 1);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const int e = l16 * 3 + k;
                        c.clq[rd][k] = (okc && e < c.n_t) ? lst[e] : (int16_t)-1;
                    }
                }
            }
            int16_t pos[2] = {-1, -1}, gs[2] = {0, 0}, ge[2] = {0, 0};
            if (c.valid) {
                st_gload(st_at(prm.plan_pos + (size_t)plan * prm.plan_stride, c.gofs), pos);
                if constexpr (LAST) {
                    st_gload(st_at(prm.plan_hgs + (size_t)plan * prm.plan_stride, c.gofs), gs);
                    st_gload(st_at(prm.plan_hge + (size_t)plan * prm.plan_stride, c.gofs), ge);
                }
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const bool live = pos[k] >= 0;
                c.live[k] = live;
                c.posz[k] = live ? (int)pos[k] : NPAD - 1;
                c.posw[k] = live ? (int)pos[k] : NPAD - 2 - (tid & 3);
                c.gsm1[k] = (live && gs[k] > 0) ? (int)gs[k] - 1 : NPAD - 1;
                c.gem1[k] = live ? (int)ge[k] - 1 : NPAD - 1;
            }
        }
        StV r0, r1;
        for (int k = 0; k < 2; ++k) {  // (lanes without hands hold zeros)
            const float w = c.live[k] ? inst_w : 0.f;
            r0.v[k] = c.pp0[k] * w;
            r1.v[k] = c.pp1[k] * w;
        }
        ST_TICK(c, 0);  // instance set-up: table entry, plan fields, root reach
        StV ev0, ev1, br0, br1;
        for (int k = 0; k < 2; ++k) { ev0.v[k] = 0.f; ev1.v[k] = 0.f; br0.v[k] = 0.f; br1.v[k] = 0.f; }
        if constexpr (!prl_fhp_runs_seat(MODE, 0)) {
            st_seat<LAST, MODE, 1, S0, S1, true>(c, R, r0, ev1, br1);
            if constexpr (MODE == PRL_FHP_UPDATE1_EVAL1) {
                // seat 1's regrets (and R.rg) are updated: its value (-> br0) and best response under the NEW strategy
                if (c.valid) StUp<LAST, MODE, PRL_FHP_EVAL, 1, S0, PRL_SRC_STRAT32, 0, 2>::run(c, R, br0, br1);
            }
        } else {
            st_seat<LAST, MODE, 0, S0, S1, true>(c, R, r1, ev0, br0);
            if constexpr (prl_fhp_runs_seat(MODE, 1)) {
                prl_sync_lds();  // the work area is reused
                st_seat<LAST, MODE, 1, S0, S1, false>(c, R, r0, ev1, br1);
            }
        }
        ST_TICK(c, 4);  // value walk(s) with the updates
        if (c.valid) {
            constexpr bool BOTH = prl_fhp_runs_seat(MODE, 0) && prl_fhp_runs_seat(MODE, 1);
            constexpr int SEAT = prl_fhp_runs_seat(MODE, 0) ? 0 : 1;
            constexpr int NV = prl_fhp_out_width(MODE);
            FhpF rowv[NV];
            if constexpr (BOTH) {
                rowv[0] = ev0.v; rowv[1] = ev1.v;
                if constexpr (prl_fhp_with_br(MODE)) { rowv[2] = br0.v; rowv[3] = br1.v; }
            } else if constexpr (MODE == PRL_FHP_UPDATE1_EVAL1) {
                rowv[0] = ev1.v; rowv[1] = br0.v; rowv[2] = br1.v;
            } else {
                rowv[0] = SEAT == 0 ? ev0.v : ev1.v;
                if constexpr (prl_fhp_with_br(MODE)) rowv[1] = SEAT == 0 ? br0.v : br1.v;
            }
            float* o = prm.val + (size_t)val_slot * NV * prm.R;
#pragma unroll
            for (int v = 0; v < NV; ++v) st_gstore_f(st_at(o + (size_t)v * prm.R, c.gofs), rowv[v]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// launchers of this spec
// ---------------------------------------------------------------------------------------------------------------------------------
template <int S0, int S1>
static void st_launch_down_t(const PrlStParams& prm, void* stream) {
    const int grid = prm.n_inst < 4096 ? prm.n_inst : 4096;
    PRL_LAUNCH((prl_k_st_down<S0, S1>), grid, ST_THREADS, 0, stream, prm);
}
int launch_down(const PrlStParams& prm, int src0, int src1, void* stream) {
    if (prm.n_inst <= 0) return PRL_OK;
    if (prm.R != ST_R) return PRL_ERR_UNSUPPORTED;
    switch (src0 * 10 + src1) {
        case PRL_SRC_UNIFORM64 * 10 + PRL_SRC_UNIFORM64: st_launch_down_t<PRL_SRC_UNIFORM64, PRL_SRC_UNIFORM64>(prm, stream); break;
        case PRL_SRC_REGRET * 10 + PRL_SRC_UNIFORM64: st_launch_down_t<PRL_SRC_REGRET, PRL_SRC_UNIFORM64>(prm, stream); break;
        case PRL_SRC_REGRET * 10 + PRL_SRC_REGRET: st_launch_down_t<PRL_SRC_REGRET, PRL_SRC_REGRET>(prm, stream); break;
        case PRL_SRC_ARR64 * 10 + PRL_SRC_ARR64: st_launch_down_t<PRL_SRC_ARR64, PRL_SRC_ARR64>(prm, stream); break;
        case PRL_SRC_ARR32 * 10 + PRL_SRC_ARR32: st_launch_down_t<PRL_SRC_ARR32, PRL_SRC_ARR32>(prm, stream); break;
        case PRL_SRC_STRAT32 * 10 + PRL_SRC_STRAT32: st_launch_down_t<PRL_SRC_STRAT32, PRL_SRC_STRAT32>(prm, stream); break;
        case PRL_SRC_AVGF32 * 10 + PRL_SRC_AVGF32: st_launch_down_t<PRL_SRC_AVGF32, PRL_SRC_AVGF32>(prm, stream); break;
        default: return PRL_ERR_UNSUPPORTED;
    }
    return PRL_OK;
}

template <bool LAST, int MODE, int S0, int S1, int STEADY = 0>
static void st_launch_pass_t(const PrlStParams& prm, int grid, void* stream) {
    static_assert(st_lds_bytes<LAST>() <= 160 * 1024, "the terminal vectors of this shape must fit the CU's LDS");
    PRL_LAUNCH((prl_k_st_pass<LAST, MODE, S0, S1, STEADY>), grid, ST_THREADS, st_lds_bytes<LAST>(), stream, prm);
}
template <bool LAST>
static int launch_pass_l(const PrlStParams& prm, int mode, int src0, int src1, void* stream) {
    if (prm.n_inst <= 0) return PRL_OK;
    if (prm.R != ST_R) return PRL_ERR_UNSUPPORTED;
    const int grid = prm.n_inst < prm.max_grid ? prm.n_inst : prm.max_grid;
    const int steady = prm.iter == 0 ? 0 : (prm.variant == PRL_CFR_PLUS && prm.avg_mode == 2 && prm.avgsum_mask == 0) ? (prm.avg32 ? 4 : 1) : 0;
    constexpr int RG = PRL_SRC_REGRET, U64 = PRL_SRC_UNIFORM64;
    switch (mode * 100 + src0 * 10 + src1) {
        case PRL_FHP_UPDATE0 * 100 + U64 * 10 + U64: st_launch_pass_t<LAST, PRL_FHP_UPDATE0, U64, U64>(prm, grid, stream); break;
        case PRL_FHP_UPDATE1 * 100 + RG * 10 + U64: st_launch_pass_t<LAST, PRL_FHP_UPDATE1, RG, U64>(prm, grid, stream); break;
        case PRL_FHP_UPDATE0 * 100 + RG * 10 + RG: st_launch_pass_t<LAST, PRL_FHP_UPDATE0, RG, RG>(prm, grid, stream); break;
        case PRL_FHP_UPDATE1 * 100 + RG * 10 + RG: st_launch_pass_t<LAST, PRL_FHP_UPDATE1, RG, RG>(prm, grid, stream); break;
        case PRL_FHP_UPDATE0_EVAL * 100 + RG * 10 + RG: st_launch_pass_t<LAST, PRL_FHP_UPDATE0_EVAL, RG, RG>(prm, grid, stream); break;
        case PRL_FHP_UPDATE0_BR * 100 + RG * 10 + RG:
            if (steady == 1) st_launch_pass_t<LAST, PRL_FHP_UPDATE0_BR, RG, RG, 1>(prm, grid, stream);
            else if (steady == 4) st_launch_pass_t<LAST, PRL_FHP_UPDATE0_BR, RG, RG, 4>(prm, grid, stream);
            else st_launch_pass_t<LAST, PRL_FHP_UPDATE0_BR, RG, RG>(prm, grid, stream);
            break;
        case PRL_FHP_UPDATE1_EVAL1 * 100 + RG * 10 + RG:
            if (steady == 1) st_launch_pass_t<LAST, PRL_FHP_UPDATE1_EVAL1, RG, RG, 1>(prm, grid, stream);
            else if (steady == 4) st_launch_pass_t<LAST, PRL_FHP_UPDATE1_EVAL1, RG, RG, 4>(prm, grid, stream);
            else st_launch_pass_t<LAST, PRL_FHP_UPDATE1_EVAL1, RG, RG>(prm, grid, stream);
            break;
        case PRL_FHP_EVAL0 * 100 + RG * 10 + RG: st_launch_pass_t<LAST, PRL_FHP_EVAL0, RG, RG>(prm, grid, stream); break;
        case PRL_FHP_EVAL * 100 + U64 * 10 + U64: st_launch_pass_t<LAST, PRL_FHP_EVAL, U64, U64>(prm, grid, stream); break;
        case PRL_FHP_EVAL * 100 + RG * 10 + RG: st_launch_pass_t<LAST, PRL_FHP_EVAL, RG, RG>(prm, grid, stream); break;
        case PRL_FHP_EVAL * 100 + PRL_SRC_ARR64 * 10 + PRL_SRC_ARR64: st_launch_pass_t<LAST, PRL_FHP_EVAL, PRL_SRC_ARR64, PRL_SRC_ARR64>(prm, grid, stream); break;
        case PRL_FHP_EVAL * 100 + PRL_SRC_STRAT32 * 10 + PRL_SRC_STRAT32: st_launch_pass_t<LAST, PRL_FHP_EVAL, PRL_SRC_STRAT32, PRL_SRC_STRAT32>(prm, grid, stream); break;
        case PRL_FHP_EVAL * 100 + PRL_SRC_ARR32 * 10 + PRL_SRC_ARR32: st_launch_pass_t<LAST, PRL_FHP_EVAL, PRL_SRC_ARR32, PRL_SRC_ARR32>(prm, grid, stream); break;
        case PRL_FHP_EVAL * 100 + PRL_SRC_AVGF32 * 10 + PRL_SRC_AVGF32: st_launch_pass_t<LAST, PRL_FHP_EVAL, PRL_SRC_AVGF32, PRL_SRC_AVGF32>(prm, grid, stream); break;
        default: return PRL_ERR_UNSUPPORTED;
    }
    return PRL_OK;
}
int launch_pass(bool last, const PrlStParams& prm, int mode, int src0, int src1, void* stream) {
    return last ? launch_pass_l<true>(prm, mode, src0, src1, stream) : launch_pass_l<false>(prm, mode, src0, src1, stream);
}

#undef ST_R
#undef ST_NL
#undef ST_NF
#undef ST_NCOLS
#undef ST_MAXA
#undef ST_NLIVE_LAST

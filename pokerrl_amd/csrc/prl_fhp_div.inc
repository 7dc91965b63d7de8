// Packed per-lane float vectors and the shared-reciprocal regret matching of the fused board pass (prl_fhp_pass.inc).
// Included inside the per-configuration namespace with FHP_SLOTS defined; also by scripts/ubench/div_check.hip, which
// compares fhp_regret_match with the generic correctly rounded division on the GPU over random and boundary operands.
// The values of a lane's FHP_SLOTS hands as one short vector: on gfx950 the element-wise float32 operations of two slots
// issue as ONE packed instruction (v_pk_add_f32 / v_pk_mul_f32; exact IEEE results per element, nothing is contracted), which
// matters because the kernel is bound by VALU issue. The emulator build gets the same interface from a plain struct.
#if defined(PRL_EMU)
struct FhpF {
    float e[FHP_SLOTS];
    float& operator[](int k) { return e[k]; }
    const float& operator[](int k) const { return e[k]; }
};
#define FHP_VOP(op) \
    inline FhpF operator op(const FhpF& a, const FhpF& b) { FhpF r; for (int k = 0; k < FHP_SLOTS; ++k) r.e[k] = a.e[k] op b.e[k]; return r; } \
    inline FhpF operator op(const FhpF& a, float b) { FhpF r; for (int k = 0; k < FHP_SLOTS; ++k) r.e[k] = a.e[k] op b; return r; } \
    inline FhpF operator op(float a, const FhpF& b) { FhpF r; for (int k = 0; k < FHP_SLOTS; ++k) r.e[k] = a op b.e[k]; return r; }
FHP_VOP(+) FHP_VOP(-) FHP_VOP(*)
#undef FHP_VOP
inline FhpF operator-(const FhpF& a) { FhpF r; for (int k = 0; k < FHP_SLOTS; ++k) r.e[k] = -a.e[k]; return r; }
#else
typedef float FhpF __attribute__((ext_vector_type(FHP_SLOTS)));
#endif

// ---------------------------------------------------------------------------------------------------------------------
// Regret matching of one node, all slots of the lane: q[i] = sum > 0 ? t[i] / sum : 1 / A with CORRECTLY ROUNDED quotients
// (the reference divides in NumPy float32). The generic expansion of a float32 division costs 10 VALU instructions per
// quotient (2 v_div_scale, v_rcp at quarter rate, 5 fma/mul, v_div_fmas, v_div_fixup) and cannot be packed; divisions were
// ~30 % of this kernel's VALU issue. The fast path shares the reciprocal of the common denominator between the A quotients
// of a node and runs the refinement as PACKED fma over the lane's slots -- exactly the instruction sequence of the generic
// expansion minus its range scaling / special-case fix-up, which are the identity when no operand, quotient or residual
// leaves the normal range (the residuals a - b q are then exact). Two sufficient boxes are used:
//   * per value (fhp_box_*): every t is 0 or in [2^-40, 2^18]  =>  sum in [2^-40, 2^20), quotients 0 or >= 2^-60; a wave
//     checks all the regrets it loaded for a board once and then takes the fast path at every node of the board;
//   * per node (fhp_node_in_box): 2^-35 <= sum <= 2^30 and every t[i] is 0 or >= 2^-33 sum.
// A wave with any lane outside the box takes the generic divisions, so the result is the correctly rounded quotient in
// every case (scripts/ubench/div_check.hip compares both paths on the GPU over random and boundary operands).
// STATUS: built only with -DFHP_DIV_FAST (python -m pokerrl_amd.build --variant fastdiv FHP_DIV_FAST). Measured on MI355X
// (profiles/r01_experiments.txt): in isolation the packed path is 1.6-1.9x faster than the generic divisions and 99.99 % of
// the waves of a real solve are inside the box, VALU instructions of the board pass drop by 11 % -- and the pass gets 3-5 %
// SLOWER: at 2.75 waves per SIMD the pass is bound by each wave's dependent-instruction chain, not by VALU throughput
// (VALU busy 46 %), and the shared reciprocal turns 4-6 independent division chains into one longer chain.
// ---------------------------------------------------------------------------------------------------------------------
#if defined(PRL_EMU)
inline FhpF fhp_fma(const FhpF& a, const FhpF& b, const FhpF& c) { FhpF r; for (int k = 0; k < FHP_SLOTS; ++k) r.e[k] = __builtin_fmaf(a.e[k], b.e[k], c.e[k]); return r; }
inline float fhp_rcp(float x) { return 1.0f / x; }
#else
PRL_DEV PRL_INLINE FhpF fhp_fma(FhpF a, FhpF b, FhpF c) { return __builtin_elementwise_fma(a, b, c); }
PRL_DEV PRL_INLINE float fhp_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
#endif
PRL_DEV PRL_INLINE unsigned fhp_bits(float x) { unsigned u; __builtin_memcpy(&u, &x, 4); return u; }

// per-value box: non-negative floats order like their bit patterns; bits - 1 wraps 0 to the maximum
struct FhpBox { unsigned umin, umax; };
PRL_DEV PRL_INLINE FhpBox fhp_box_empty() { FhpBox b; b.umin = 0xFFFFFFFFu; b.umax = 0u; return b; }
PRL_DEV PRL_INLINE void fhp_box_add(FhpBox& b, float t) {
    const unsigned u = fhp_bits(t);
    b.umax = u > b.umax ? u : b.umax;
    b.umin = u - 1u < b.umin ? u - 1u : b.umin;
}
PRL_DEV PRL_INLINE bool fhp_box_ok(const FhpBox& b) { return b.umax <= 0x48800000u /* 2^18 */ && b.umin >= 0x2B800000u - 1u /* 2^-40 */; }

// MA (deduced): the action bound of the caller's shape, the first extent of its per-action arrays (PrlFhpDerive::MAX_A; 3 in the board pass)
template <int A, int MA>
PRL_DEV PRL_INLINE bool fhp_node_in_box(const float (&t)[MA][FHP_SLOTS], const float (&sum)[FHP_SLOTS]) {
    static_assert(A <= 3 && A <= MA, "the per-node box bounds min t / sum for a sum of at most three addends: nodes with more actions take fhp_regret_match_generic");
    unsigned ok = 1u;
    for (int k = 0; k < FHP_SLOTS; ++k) {
        const float b = sum[k] > 0.f ? sum[k] : 1.f;
        unsigned m = fhp_bits(t[0][k]) - 1u;
        for (int i = 1; i < A; ++i) { const unsigned u = fhp_bits(t[i][k]) - 1u; m = u < m ? u : m; }
        ok &= (unsigned)(m >= fhp_bits(b * 0x1p-33f) - 1u) & (unsigned)(fhp_bits(b) - 0x2E000000u <= 0x4E800000u - 0x2E000000u);
    }
    return ok != 0u;
}

template <int A, int MA>
PRL_DEV PRL_INLINE void fhp_regret_match_generic(const float (&t)[MA][FHP_SLOTS], const float (&sum)[FHP_SLOTS], float (&q)[MA][FHP_SLOTS]) {
    static_assert(A <= MA, "more actions than the shape's bound");
    const float unif = (float)(1.0 / (double)A);
    for (int i = 0; i < A; ++i)
        for (int k = 0; k < FHP_SLOTS; ++k) q[i][k] = sum[k] > 0.f ? t[i][k] / sum[k] : unif;
}

template <int A, int MA>
PRL_DEV PRL_INLINE void fhp_regret_match_fast(const float (&t)[MA][FHP_SLOTS], const float (&sum)[FHP_SLOTS], float (&q)[MA][FHP_SLOTS]) {
    static_assert(A <= 3 && A <= MA, "the boxes above are derived for at most three addends");
    const float unif = (float)(1.0 / (double)A);
    FhpF b, y;
    bool pos[FHP_SLOTS];
    for (int k = 0; k < FHP_SLOTS; ++k) {
        pos[k] = sum[k] > 0.f;
        b[k] = pos[k] ? sum[k] : 1.f;  // all t[i] are 0 then: the quotients are discarded
        y[k] = fhp_rcp(b[k]);
    }
    const FhpF e = fhp_fma(-b, y, FhpF{} + 1.0f);
    y = fhp_fma(e, y, y);
    for (int i = 0; i < A; ++i) {
        FhpF n;
        for (int k = 0; k < FHP_SLOTS; ++k) n[k] = t[i][k];
        FhpF qq = n * y;
        FhpF r = fhp_fma(-b, qq, n);
        qq = fhp_fma(r, y, qq);
        r = fhp_fma(-b, qq, n);
        qq = fhp_fma(r, y, qq);
        for (int k = 0; k < FHP_SLOTS; ++k) q[i][k] = pos[k] ? qq[k] : unif;
    }
}

// fast: WAVE-UNIFORM, true only if every lane of the wave is inside one of the boxes for this node
// (a node with four actions always divides generically: the street pass, the only walk that has such nodes, calls fhp_regret_match_generic itself)
template <int A, int MA>
PRL_DEV PRL_INLINE void fhp_regret_match(const float (&t)[MA][FHP_SLOTS], const float (&sum)[FHP_SLOTS], float (&q)[MA][FHP_SLOTS], bool fast) {
    if constexpr (A <= 3) { if (fast) { fhp_regret_match_fast<A>(t, sum, q); return; } }
    fhp_regret_match_generic<A>(t, sum, q);
}

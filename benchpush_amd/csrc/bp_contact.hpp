// Lane-local contact arithmetic shared by substep() (bp_physics.hpp, one env per wavefront) and substep_pair() (bp_physics_pair.hpp, two envs per
// wavefront): the hint word of the narrow phase, cpArbiterUpdate on the owning lane, cpSpaceArbiterSetFilter and cpArbiterPreStep -- one text each.
// The rule of this file: lane-local only.  Inputs are values and an ArbReg &, outputs are values or references -- no lane index, no ballot, no LDS or
// global pointer, no EnvCtx / LdsCtx / PW, no profile stamp.  Addressing (which array, which offset, in which order the loads are issued), wave-level
// control and the stamps stay with the callers, which differ there on purpose.  Everything is __forceinline__ and every kernel has to compile to the
// code it compiled to when the callers spelled the block out (tools/isa_compare.py; the operation order is part of the contract: -ffp-contract=off,
// bit-pinned to the oracle).  That is why arbiter_update takes its d2 arguments by reference -- by value the same source moved 14 kernels -- and why the
// closest-feature normal, ContactPoints, the warm start and the solver pass are still spelled out in both callers (profiles/contact_share/README.md).
#pragma once
#include "bp_device.hpp"

struct ArbReg {
    unsigned key, stamp, h0, h1;
    int state, count, level, rank;
    double jn0, jt0, jn1, jt1;
    d2 n, r1_0, r2_0, r1_1, r2_1;
    double ma, ia, mb, ib;
    double e, u;               // elasticity / friction products of the two shapes (cpArbiterUpdate)
    int slotA, slotB;          // velocity slots of the two bodies
};

struct Manifold { int count; d2 n; d2 p1_0, p2_0, p1_1, p2_1; unsigned h0, h1; };

__device__ __forceinline__ void apply_contact_impulses(const ArbReg &A, int c, d2 &va, double &wa, d2 &vb, double &wb, d2 j)
{
    const d2 r1 = c ? A.r1_1 : A.r1_0, r2 = c ? A.r2_1 : A.r2_0;
    const d2 jn = vneg(j);
    va = vadd(va, vmul(jn, A.ma));
    wa += A.ia * vcross(r1, jn);
    vb = vadd(vb, vmul(j, A.mb));
    wb += A.ib * vcross(r2, j);
}

// The pair's next hint word: the winners of both sides are the next sub-step's cached planes.
__device__ __forceinline__ unsigned long long hint_word(const int iA, const int iB, const int jA, const int jB, const int nA, const int nB,
                                                        const bool useA, const double smax, const double rsum)
{
    return (unsigned long long)((unsigned)iA | ((unsigned)iB << 5) | ((unsigned)jA << 10) | ((unsigned)jB << 15) |
                                ((unsigned)nA << 20) | ((unsigned)nB << 25)) |
           HW_HAS_A | HW_HAS_B | (useA ? 0ull : HW_PRIM_B) | ((smax > rsum) ? 0ull : HW_BOTH);
}

// ---- 4c. cpArbiterUpdate on the lane that owns the pair's arbiter -------------------------------------------------------------------------------------
// A lane that adopts a pair nobody owned: masses (m1, m2 = mass rows of the two bodies) and material products (q1, q2 = their prop rows) stay with the arbiter.
__device__ __forceinline__ void arbiter_adopt(ArbReg &A, const double4 m1, const double4 m2, const double4 q1, const double4 q2)
{
    A.state = ARB_FIRST; A.count = 0; A.h0 = A.h1 = 0; A.jn0 = A.jt0 = A.jn1 = A.jt1 = 0.0;
    A.ma = m1.x; A.ia = m1.y; A.mb = m2.x; A.ib = m2.y;
    A.e = q1.y * q2.y; A.u = q1.z * q2.z;
}

// The delivered manifold (normal mn, contact points mp1x / mp2x, feature hashes mh0 / mh1, mcount contacts) replaces the arbiter's contacts; an accumulated
// impulse is carried over to the new contact with the same hash.  pa / pb: positions of the two bodies.
__device__ __forceinline__ void arbiter_update(ArbReg &A, const d2 &mn, const d2 &mp10, const d2 &mp20, const d2 &mp11, const d2 &mp21,
                                               const unsigned mh0, const unsigned mh1, const int mcount, const d2 &pa, const d2 &pb, const unsigned now)
{
    double njn0 = 0.0, njt0 = 0.0, njn1 = 0.0, njt1 = 0.0;
    if (A.count > 0 && A.h0 == mh0) { njn0 = A.jn0; njt0 = A.jt0; }
    if (A.count > 1 && A.h1 == mh0) { njn0 = A.jn1; njt0 = A.jt1; }
    if (mcount > 1) {
        if (A.count > 0 && A.h0 == mh1) { njn1 = A.jn0; njt1 = A.jt0; }
        if (A.count > 1 && A.h1 == mh1) { njn1 = A.jn1; njt1 = A.jt1; }
    }
    A.jn0 = njn0; A.jt0 = njt0; A.jn1 = njn1; A.jt1 = njt1;
    A.h0 = mh0; A.h1 = mh1;
    A.r1_0 = vsub(mp10, pa); A.r2_0 = vsub(mp20, pb);
    A.r1_1 = vsub(mp11, pa); A.r2_1 = vsub(mp21, pb);
    A.count = mcount;
    A.n = mn;
    if (A.state == ARB_CACHED) A.state = ARB_FIRST;
    A.stamp = now;
}

// ---- 5. cpSpaceArbiterSetFilter ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void arbiter_filter(ArbReg &A, const unsigned now, const int persistence)
{
    if (A.key != ARB_FREE_KEY) {
        const unsigned ticks = now - A.stamp;
        if (ticks >= 1u && A.state != ARB_CACHED) A.state = ARB_CACHED;
        if (ticks >= (unsigned)persistence) A.key = ARB_FREE_KEY;
    }
}

// ---- 6a. cpArbiterPreStep of one contact (r1, r2) ------------------------------------------------------------------------------------------------------
// bias is the bias velocity times dt: the callers divide by dt when it is not a zero (a signed zero / dt is that zero).
__device__ __forceinline__ void prestep_contact(const DevParams &P, const ArbReg &A, const d2 r1, const d2 r2, const d2 n, const d2 t, const d2 body_delta,
                                                const d2 va, const d2 vb, const double wa, const double wb,
                                                double &nMass, double &tMass, double &bias, double &jBias, double &bounce)
{
    const double rcn1 = vcross(r1, n), rcn2 = vcross(r2, n);
    nMass = 1.0 / ((A.ma + A.ia * rcn1 * rcn1) + (A.mb + A.ib * rcn2 * rcn2));
    const double rct1 = vcross(r1, t), rct2 = vcross(r2, t);
    tMass = 1.0 / ((A.ma + A.ia * rct1 * rct1) + (A.mb + A.ib * rct2 * rct2));
    const double dist = vdot(vadd(vsub(r2, r1), body_delta), n);
    bias = -P.bias_coef * fmin(0.0, dist + P.slop);
    jBias = 0.0;
    const d2 v1 = vadd(va, vmul(vperp(r1), wa));
    const d2 v2 = vadd(vb, vmul(vperp(r2), wb));
    bounce = vdot(vsub(v2, v1), n) * A.e;
}

// x is -0.0.  (The register path of the solver adds zero impulses to an infinite-mass body's velocity: x + (+-0) == x bit for bit unless x is a negative zero.)
__device__ __forceinline__ bool is_negzero(const double x) { return (((unsigned)__double2hiint(x) ^ 0x80000000u) | (unsigned)__double2loint(x)) == 0u; }

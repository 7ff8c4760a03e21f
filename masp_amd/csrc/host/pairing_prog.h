// The Miller loop of the GPU batch verifier as straight-line PROGRAMS over Fp.
//
// One pair's Miller loop is a chain of ~10 000 dependent 384-bit products when a single lane walks the Fp12 tower; on a
// lone wave each costs ~2.4 us.  But inside one iteration almost everything is independent: the 36 base-field products of
// the Fp12 squaring, the 39 of the sparse line multiplication, the dozen of the point doubling.  So the iteration is not
// written as device code at all: the formulas (the same ones as host/pairing.h: projective doubling / mixed addition on
// the twist, sparse line (c0, c1 v, c2 v w), Karatsuba tower) are written ONCE below as templates over the base field,
// instantiated with a symbolic type that records every Fp operation into a DAG, and the DAG is levelled (ASAP) into
// steps of mutually independent operations with values living in numbered 48-byte slots.  The device kernel
// (device/pairing.hpp) is then a tiny interpreter: one WAVE per pair, slots in LDS, lane k of the wave executes the k-th
// operation of the current step — a doubling iteration is ~6 steps that contain products instead of ~135 products in a row.
// The same program runs on the host interpreter below, which is how it is checked against host/pairing.h without a GPU
// (masp_host_pairing_program_selftest, tests/test_pairing_program.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <tuple>
#include <vector>

#include "pairing.h"

namespace masp_host {
namespace prog {

enum Op : uint32_t { OP_MUL = 0, OP_ADD = 1, OP_SUB = 2, OP_MOV = 3 };

// ---- fixed slots (the loop-carried state of one pair) -------------------------------------------------------
enum : int {
    SLOT_ZERO = 0,
    SLOT_F = 1,    // 12: a.a.a a.a.b a.b.a a.b.b a.c.a a.c.b b.a.a b.a.b b.b.a b.b.b b.c.a b.c.b
    SLOT_T = 13,   // 6: X.a X.b Y.a Y.b Z.a Z.b
    SLOT_P = 19,   // 2: xp yp
    SLOT_Q = 21,   // 4: xq.a xq.b yq.a yq.b
    SLOT_Y = 13,   // Fp12 product program: second operand in 13..24
    N_FIXED = 25,
};

// ---- tracer ---------------------------------------------------------------------------------------------------
struct Tracer {
    struct Node {
        int op;  // -1: input (a = fixed slot)
        int a, b;
    };
    std::vector<Node> nodes;
    std::map<std::tuple<int, int, int>, int> cse;
    int input(int slot) {
        auto key = std::make_tuple(-1, slot, 0);
        auto it = cse.find(key);
        if (it != cse.end()) return it->second;
        nodes.push_back({-1, slot, 0});
        return cse[key] = (int)nodes.size() - 1;
    }
    int emit(Op op, int a, int b) {
        if ((op == OP_MUL || op == OP_ADD) && a > b) std::swap(a, b);
        auto key = std::make_tuple((int)op, a, b);
        auto it = cse.find(key);
        if (it != cse.end()) return it->second;
        nodes.push_back({(int)op, a, b});
        return cse[key] = (int)nodes.size() - 1;
    }
    static Tracer*& cur() {
        static thread_local Tracer* t = nullptr;
        return t;
    }
};
// symbolic base-field element
struct S {
    int id;
    S operator+(const S& o) const { return {Tracer::cur()->emit(OP_ADD, id, o.id)}; }
    S operator-(const S& o) const { return {Tracer::cur()->emit(OP_SUB, id, o.id)}; }
    S operator*(const S& o) const { return {Tracer::cur()->emit(OP_MUL, id, o.id)}; }
    S neg() const { return S{Tracer::cur()->input(SLOT_ZERO)} - *this; }
    S dbl() const { return *this + *this; }
    S sq() const { return *this * *this; }
};

// ---- the tower and the Miller steps, over any base field F (host/pairing.h's formulas) -----------------------------
template <class F>
struct Fp2T {
    F a, b;
    Fp2T operator+(const Fp2T& o) const { return {a + o.a, b + o.b}; }
    Fp2T operator-(const Fp2T& o) const { return {a - o.a, b - o.b}; }
    Fp2T neg() const { return {a.neg(), b.neg()}; }
    Fp2T operator*(const Fp2T& o) const {
        F t0 = a * o.a, t1 = b * o.b;
        return {t0 - t1, (a + b) * (o.a + o.b) - t0 - t1};
    }
    Fp2T sq() const { return {(a + b) * (a - b), (a * b).dbl()}; }
    Fp2T xi() const { return {a - b, a + b}; }
    Fp2T scale(const F& k) const { return {a * k, b * k}; }
};
template <class F>
struct Fp6T {
    typedef Fp2T<F> E;
    E a, b, c;
    Fp6T operator+(const Fp6T& o) const { return {a + o.a, b + o.b, c + o.c}; }
    Fp6T operator-(const Fp6T& o) const { return {a - o.a, b - o.b, c - o.c}; }
    Fp6T operator*(const Fp6T& o) const {
        E v0 = a * o.a, v1 = b * o.b, v2 = c * o.c;
        return {v0 + ((b + c) * (o.b + o.c) - v1 - v2).xi(), (a + b) * (o.a + o.b) - v0 - v1 + v2.xi(), (a + c) * (o.a + o.c) - v0 - v2 + v1};
    }
    Fp6T mul_01(const E& x0, const E& x1) const {
        E v0 = a * x0, v1 = b * x1;
        return {v0 + (c * x1).xi(), (a + b) * (x0 + x1) - v0 - v1, v1 + c * x0};
    }
    Fp6T mul_1(const E& x1) const { return {(c * x1).xi(), a * x1, b * x1}; }
    Fp6T mulv() const { return {c.xi(), a, b}; }
};
template <class F>
struct Fp12T {
    typedef Fp2T<F> E;
    Fp6T<F> a, b;
    Fp12T operator*(const Fp12T& o) const {
        Fp6T<F> t0 = a * o.a, t1 = b * o.b;
        return {t0 + t1.mulv(), (a + b) * (o.a + o.b) - t0 - t1};
    }
    Fp12T sq() const {
        Fp6T<F> ab = a * b;
        return {(a + b) * (a + b.mulv()) - ab - ab.mulv(), ab + ab};
    }
    Fp12T mul_line(const E& c0, const E& c1, const E& c2) const {
        Fp6T<F> t0 = a.mul_01(c0, c1), t1 = b.mul_1(c2);
        return {t0 + t1.mulv(), (a + b).mul_01(c0, c1 + c2) - t0 - t1};
    }
};
// ---- the final exponentiation's pieces (host/pairing.h's frobenius and Fp2 / Fp6 / Fp12 inv), over any base field ---------
// x -> x^p: conj of every Fp2 coefficient, times gamma[i] for the coefficient of w^i (g[0..4] = gamma[1..5])
template <class F>
Fp12T<F> frobenius_t(const Fp12T<F>& f, const Fp2T<F>* g) {
    auto cj = [](const Fp2T<F>& x) { return Fp2T<F>{x.a, x.b.neg()}; };
    return {{cj(f.a.a), cj(f.a.b) * g[1], cj(f.a.c) * g[3]}, {cj(f.b.a) * g[0], cj(f.b.b) * g[2], cj(f.b.c) * g[4]}};
}
// x -> x^(p^2): the coefficient of w^i times gamma[i] conj(gamma[i]), which lies in Fp (n[0..4] for i = 1..5)
template <class F>
Fp12T<F> frobenius2_t(const Fp12T<F>& f, const F* n) {
    return {{f.a.a, f.a.b.scale(n[1]), f.a.c.scale(n[3])}, {f.b.a.scale(n[0]), f.b.b.scale(n[2]), f.b.c.scale(n[4])}};
}
// f^-1 = conj(f) / (a^2 - v b^2); the Fp6 below is inverted through its Fp2 norm D, and D through its Fp norm n.  The first half
// stops at n, the only value whose inverse has to be computed; the second half finishes from 1 / n.
template <class F>
struct Fp12InvT {
    Fp2T<F> t0, t1, t2, D;
    F n;
    void first(const Fp12T<F>& f) {
        const Fp6T<F> d = f.a * f.a - (f.b * f.b).mulv();
        t0 = d.a.sq() - (d.b * d.c).xi();
        t1 = d.c.sq().xi() - d.a * d.b;
        t2 = d.b.sq() - d.a * d.c;
        D = d.a * t0 + (d.c * t1 + d.b * t2).xi();
        n = D.a.sq() + D.b.sq();
    }
    Fp12T<F> second(const Fp12T<F>& f, const F& ninv) const {
        const Fp2T<F> Di = {D.a * ninv, (D.b * ninv).neg()};
        const Fp6T<F> di = {t0 * Di, t1 * Di, t2 * Di};
        const Fp6T<F> hb = f.b * di;
        return {f.a * di, {hb.a.neg(), hb.b.neg(), hb.c.neg()}};
    }
};

template <class F>
struct MillerT {
    typedef Fp2T<F> E;
    F xp, yp;
    E xq, yq;
    E X, Y, Z;
    // T <- 2T ; f <- f * l_{T,T}(P)
    void dbl_step(Fp12T<F>& f) {
        E Y2 = Y.sq(), Z2 = Z.sq(), X2 = X.sq();
        E bz = Z2.xi();
        bz = bz + bz;
        bz = bz + bz;
        E Ee = bz + bz + bz;
        E YZ2 = Y * Z;
        YZ2 = YZ2 + YZ2;
        E X23 = X2 + X2 + X2;
        f = f.mul_line(Y2 - Ee, X23.scale(xp).neg(), YZ2.scale(yp));
        E E3 = Ee + Ee + Ee, XY = X * Y;
        E EY = Ee * Y2, E2 = Ee.sq();
        E EY2 = EY + EY, EY6 = EY2 + EY2 + EY2;
        X = (XY + XY) * (Y2 - E3);
        Y = Y2.sq() + EY6 - (E2 + E2 + E2);
        E Y2Z = Y2 * YZ2;
        Y2Z = Y2Z + Y2Z;
        Z = Y2Z + Y2Z;
    }
    // T <- T + Q ; f <- f * l_{T,Q}(P)
    void add_step(Fp12T<F>& f) {
        E N = Y - yq * Z, D = X - xq * Z;
        f = f.mul_line(N * xq - D * yq, N.scale(xp).neg(), D.scale(yp));
        E D2 = D.sq(), D3 = D2 * D, xqZ = xq * Z;
        E A = N.sq() * Z - D2 * (X + xqZ);
        E Y3 = N * (xqZ * D2 - A) - yq * Z * D3;
        X = A * D;
        Y = Y3;
        Z = Z * D3;
    }
};

// ---- program = levelled DAG --------------------------------------------------------------------------------------
struct Program {
    std::vector<uint32_t> ops;        // op | dst << 2 | a << 12 | b << 22   (slots < 1024)
    std::vector<uint32_t> step_start;  // ops of step s: [step_start[s], step_start[s + 1])
    uint32_t n_slots = 0;
    uint32_t n_mul = 0, n_mul_steps = 0;
    static uint32_t enc(uint32_t op, uint32_t dst, uint32_t a, uint32_t b) { return op | dst << 2 | a << 12 | b << 22; }
};
// outputs: (node id, fixed slot it must end up in)
// first_temp: the first slot temporaries may take (the final exponentiation keeps constants and saved values above N_FIXED)
inline Program levelize(const Tracer& t, const std::vector<std::pair<int, int>>& outputs, int first_temp = N_FIXED) {
    const int n = (int)t.nodes.size();
    std::vector<char> live(n, 0);
    std::vector<int> stack;
    for (auto& o : outputs) stack.push_back(o.first);
    while (!stack.empty()) {
        int v = stack.back();
        stack.pop_back();
        if (live[v]) continue;
        live[v] = 1;
        if (t.nodes[v].op >= 0) {
            stack.push_back(t.nodes[v].a);
            stack.push_back(t.nodes[v].b);
        }
    }
    // Steps.  A product costs ~20x an addition and a step costs its slowest operation, so all products of the same
    // product-depth go into ONE step (the early ones wait for the late ones), with the additions that feed them in cheap
    // steps of their own in between:  [adds of level 0] [products of level 1] [adds of level 1] [products of level 2] ...
    std::vector<int> step(n, 0), last_use(n, 0), md(n, 0), ad(n, 0);
    int max_md = 0;
    for (int v = 0; v < n; ++v) {
        if (!live[v] || t.nodes[v].op < 0) continue;
        const int a = t.nodes[v].a, b = t.nodes[v].b;
        if (t.nodes[v].op == OP_MUL) {
            md[v] = std::max(md[a], md[b]) + 1;
        } else {
            md[v] = std::max(md[a], md[b]);
            // depth among the additions of this level (an operand of a lower level, or a product of this level, counts 0)
            auto dep = [&](int x) { return (t.nodes[x].op >= 0 && t.nodes[x].op != OP_MUL && md[x] == md[v]) ? ad[x] : 0; };
            ad[v] = std::max(dep(a), dep(b)) + 1;
        }
        max_md = std::max(max_md, md[v]);
    }
    std::vector<int> add_depth(max_md + 1, 0);
    for (int v = 0; v < n; ++v)
        if (live[v] && t.nodes[v].op >= 0 && t.nodes[v].op != OP_MUL) add_depth[md[v]] = std::max(add_depth[md[v]], ad[v]);
    std::vector<int> mul_step(max_md + 2, 0);  // step of the products of level L (L >= 1); additions of level L follow it
    int max_step = 0;
    {
        int cur = add_depth[0];                // additions of level 0: steps 1 .. add_depth[0]
        for (int L = 1; L <= max_md; ++L) {
            mul_step[L] = ++cur;
            cur += add_depth[L];
        }
        max_step = cur;
    }
    for (int v = 0; v < n; ++v) {
        if (!live[v] || t.nodes[v].op < 0) continue;
        step[v] = t.nodes[v].op == OP_MUL ? mul_step[md[v]] : (md[v] == 0 ? 0 : mul_step[md[v]]) + ad[v];
    }
    const int mov_step = max_step + 1;  // the outputs move into their fixed slots after every read of the old state
    for (int v = 0; v < n; ++v)
        if (live[v] && t.nodes[v].op >= 0) {
            last_use[t.nodes[v].a] = std::max(last_use[t.nodes[v].a], step[v]);
            last_use[t.nodes[v].b] = std::max(last_use[t.nodes[v].b], step[v]);
        }
    for (auto& o : outputs) last_use[o.first] = mov_step;
    // slots: inputs sit in their fixed slots; temporaries come from a free list; a slot is released only AFTER the step of
    // its value's last reader, so no step reads and writes the same slot (lanes run the ops of a step in no order)
    std::vector<int> slot(n, -1);
    std::vector<int> free_list;
    int next_slot = first_temp;
    std::vector<std::vector<int>> by_step(mov_step + 1), expiring(mov_step + 2);
    for (int v = 0; v < n; ++v) {
        if (!live[v]) continue;
        if (t.nodes[v].op < 0)
            slot[v] = t.nodes[v].a;
        else
            by_step[step[v]].push_back(v);
    }
    Program P;
    P.step_start.push_back(0);
    for (int s = 1; s <= max_step; ++s) {
        bool has_mul = false;
        for (int v : by_step[s]) {
            if (free_list.empty())
                slot[v] = next_slot++;
            else {
                slot[v] = free_list.back();
                free_list.pop_back();
            }
            expiring[last_use[v]].push_back(v);
            P.ops.push_back(Program::enc((uint32_t)t.nodes[v].op, (uint32_t)slot[v], (uint32_t)slot[t.nodes[v].a], (uint32_t)slot[t.nodes[v].b]));
            if (t.nodes[v].op == OP_MUL) {
                ++P.n_mul;
                has_mul = true;
            }
        }
        if (has_mul) ++P.n_mul_steps;
        P.step_start.push_back((uint32_t)P.ops.size());
        for (int v : expiring[s]) free_list.push_back(slot[v]);
    }
    for (auto& o : outputs) P.ops.push_back(Program::enc(OP_MOV, (uint32_t)o.second, (uint32_t)slot[o.first], 0));
    P.step_start.push_back((uint32_t)P.ops.size());
    P.n_slots = (uint32_t)next_slot;
    return P;
}

// ---- the three programs ---------------------------------------------------------------------------------------------
struct PairingPrograms {
    Program dbl;   // f <- f^2 * l_{T,T}(P),  T <- 2T
    Program add;   // f <- f   * l_{T,Q}(P),  T <- T + Q
    Program mul12; // f <- f * y   (y in slots SLOT_Y .. SLOT_Y + 11): the product tree over the pairs
    uint32_t n_slots = 0;
};
namespace detail {
inline Fp12T<S> sym_f(Tracer& t, int base) {
    S v[12];
    for (int i = 0; i < 12; ++i) v[i] = S{t.input(base + i)};
    return {{{v[0], v[1]}, {v[2], v[3]}, {v[4], v[5]}}, {{v[6], v[7]}, {v[8], v[9]}, {v[10], v[11]}}};
}
inline void out_f(std::vector<std::pair<int, int>>& o, const Fp12T<S>& f) {
    const S v[12] = {f.a.a.a, f.a.a.b, f.a.b.a, f.a.b.b, f.a.c.a, f.a.c.b, f.b.a.a, f.b.a.b, f.b.b.a, f.b.b.b, f.b.c.a, f.b.c.b};
    for (int i = 0; i < 12; ++i) o.push_back({v[i].id, SLOT_F + i});
}
inline MillerT<S> sym_pair(Tracer& t) {
    auto in = [&](int s) { return S{t.input(s)}; };
    MillerT<S> m;
    m.xp = in(SLOT_P);
    m.yp = in(SLOT_P + 1);
    m.xq = {in(SLOT_Q), in(SLOT_Q + 1)};
    m.yq = {in(SLOT_Q + 2), in(SLOT_Q + 3)};
    m.X = {in(SLOT_T), in(SLOT_T + 1)};
    m.Y = {in(SLOT_T + 2), in(SLOT_T + 3)};
    m.Z = {in(SLOT_T + 4), in(SLOT_T + 5)};
    return m;
}
inline void out_t(std::vector<std::pair<int, int>>& o, const MillerT<S>& m) {
    const S v[6] = {m.X.a, m.X.b, m.Y.a, m.Y.b, m.Z.a, m.Z.b};
    for (int i = 0; i < 6; ++i) o.push_back({v[i].id, SLOT_T + i});
}
}  // namespace detail
inline const PairingPrograms& pairing_programs() {
    static const PairingPrograms P = [] {
        PairingPrograms pp;
        {
            Tracer t;
            Tracer::cur() = &t;
            Fp12T<S> f = detail::sym_f(t, SLOT_F).sq();
            MillerT<S> m = detail::sym_pair(t);
            m.dbl_step(f);
            std::vector<std::pair<int, int>> outs;
            detail::out_f(outs, f);
            detail::out_t(outs, m);
            pp.dbl = levelize(t, outs);
        }
        {
            Tracer t;
            Tracer::cur() = &t;
            Fp12T<S> f = detail::sym_f(t, SLOT_F);
            MillerT<S> m = detail::sym_pair(t);
            m.add_step(f);
            std::vector<std::pair<int, int>> outs;
            detail::out_f(outs, f);
            detail::out_t(outs, m);
            pp.add = levelize(t, outs);
        }
        {
            Tracer t;
            Tracer::cur() = &t;
            Fp12T<S> f = detail::sym_f(t, SLOT_F) * detail::sym_f(t, SLOT_Y);
            std::vector<std::pair<int, int>> outs;
            detail::out_f(outs, f);
            pp.mul12 = levelize(t, outs);
        }
        Tracer::cur() = nullptr;
        pp.n_slots = std::max(pp.dbl.n_slots, std::max(pp.add.n_slots, pp.mul12.n_slots));
        return pp;
    }();
    return P;
}

// ---- host interpreter (reference semantics of the device kernel) ------------------------------------------------------
inline void run_program(const Program& P, bls::Fp* slots) {
    for (size_t s = 0; s + 1 < P.step_start.size(); ++s)
        for (uint32_t k = P.step_start[s]; k < P.step_start[s + 1]; ++k) {
            const uint32_t w = P.ops[k], op = w & 3, dst = (w >> 2) & 1023, a = (w >> 12) & 1023, b = (w >> 22) & 1023;
            slots[dst] = op == OP_MUL ? slots[a] * slots[b] : op == OP_ADD ? slots[a] + slots[b] : op == OP_SUB ? slots[a] - slots[b] : slots[a];
        }
}
// Miller loop of one pair through the programs, as the device runs it: f_{|x|,Q}(P) conjugated (host/pairing.h's convention)
inline bls::Fp12 miller_by_program(const bls::G1A& Pt, const bls::G2A& Q) {
    const PairingPrograms& pp = pairing_programs();
    std::vector<bls::Fp> sl(pp.n_slots, bls::Fp::zero());
    sl[SLOT_F] = bls::Fp::one();
    sl[SLOT_T] = Q.x.a; sl[SLOT_T + 1] = Q.x.b; sl[SLOT_T + 2] = Q.y.a; sl[SLOT_T + 3] = Q.y.b; sl[SLOT_T + 4] = bls::Fp::one();
    sl[SLOT_P] = Pt.x; sl[SLOT_P + 1] = Pt.y;
    sl[SLOT_Q] = Q.x.a; sl[SLOT_Q + 1] = Q.x.b; sl[SLOT_Q + 2] = Q.y.a; sl[SLOT_Q + 3] = Q.y.b;
    const uint64_t xabs = 0xd201000000010000ull;
    for (int b = 62; b >= 0; --b) {
        run_program(pp.dbl, sl.data());      // (squaring f = 1 in the first iteration is harmless)
        if ((xabs >> b) & 1) run_program(pp.add, sl.data());
    }
    const bls::Fp* f = &sl[SLOT_F];
    bls::Fp12 r = {{{f[0], f[1]}, {f[2], f[3]}, {f[4], f[5]}}, {{f[6], f[7]}, {f[8], f[9]}, {f[10], f[11]}}};
    return r.conj();
}

// ---- the final exponentiation as programs -------------------------------------------------------------------------------
// bls::final_exp (host/pairing.h) is a fixed sequence of Fp12 products, squarings, Frobenius maps, conjugations and one
// inversion.  Each of those is a program here; the sequence itself is a schedule (final_exp_schedule below) that the host
// interpreter and the device kernel k_final_exp (device/pairing.hpp) both walk.  Slots:
//   0 ZERO | 1..12 F | 13..24 Y (second operand; between the halves of the inversion t0 t1 t2 D n) |
//   25..34 gamma[1..5] | 35..39 gamma[i] conj(gamma[i]) | 40..75 three saved values of 12 | temporaries
enum : int {
    FE_T0 = SLOT_Y,          // 6: t0 t1 t2 of the Fp6 inversion
    FE_D = SLOT_Y + 6,       // 2: its Fp2 norm
    FE_N = SLOT_Y + 8,       // 1: the Fp norm, replaced by its inverse between the halves
    FE_GAMMA = 25,           // 10
    FE_NORM = 35,            // 5
    FE_BANK = 40,            // 3 x 12
    FE_N_BANKS = 3,
    FE_FIRST_TEMP = FE_BANK + 12 * FE_N_BANKS,
};
struct FinalExpPrograms {
    Program mul;    // F <- F * Y
    Program sq;     // F <- F^2
    Program frob;   // F <- F^p
    Program frob2;  // F <- F^(p^2)
    Program inv1;   // F -> t0 t1 t2 D n (FE_T0 .. FE_N); F stays
    Program inv2;   // F <- F^-1 from those, with 1 / n in FE_N
    uint32_t n_slots = 0;
    const Program* all(int i) const {
        const Program* p[6] = {&mul, &sq, &frob, &frob2, &inv1, &inv2};
        return p[i];
    }
};
inline const FinalExpPrograms& final_exp_programs() {
    static const FinalExpPrograms P = [] {
        FinalExpPrograms fp;
        typedef std::vector<std::pair<int, int>> Outs;
        auto in = [](Tracer& t, int s) { return S{t.input(s)}; };
        auto trace = [&](Program& dst, auto&& body) {
            Tracer t;
            Tracer::cur() = &t;
            Outs outs;
            body(t, outs);
            dst = levelize(t, outs, FE_FIRST_TEMP);
        };
        trace(fp.mul, [&](Tracer& t, Outs& o) { detail::out_f(o, detail::sym_f(t, SLOT_F) * detail::sym_f(t, SLOT_Y)); });
        trace(fp.sq, [&](Tracer& t, Outs& o) { detail::out_f(o, detail::sym_f(t, SLOT_F).sq()); });
        trace(fp.frob, [&](Tracer& t, Outs& o) {
            Fp2T<S> g[5];
            for (int i = 0; i < 5; ++i) g[i] = {in(t, FE_GAMMA + 2 * i), in(t, FE_GAMMA + 2 * i + 1)};
            detail::out_f(o, frobenius_t(detail::sym_f(t, SLOT_F), g));
        });
        trace(fp.frob2, [&](Tracer& t, Outs& o) {
            S n[5] = {in(t, FE_NORM), in(t, FE_NORM + 1), in(t, FE_NORM + 2), in(t, FE_NORM + 3), in(t, FE_NORM + 4)};
            detail::out_f(o, frobenius2_t(detail::sym_f(t, SLOT_F), n));
        });
        trace(fp.inv1, [&](Tracer& t, Outs& o) {
            Fp12InvT<S> h;
            h.first(detail::sym_f(t, SLOT_F));
            const S v[9] = {h.t0.a, h.t0.b, h.t1.a, h.t1.b, h.t2.a, h.t2.b, h.D.a, h.D.b, h.n};
            for (int i = 0; i < 9; ++i) o.push_back({v[i].id, FE_T0 + i});
        });
        trace(fp.inv2, [&](Tracer& t, Outs& o) {
            Fp12InvT<S> h;
            h.t0 = {in(t, FE_T0), in(t, FE_T0 + 1)};
            h.t1 = {in(t, FE_T0 + 2), in(t, FE_T0 + 3)};
            h.t2 = {in(t, FE_T0 + 4), in(t, FE_T0 + 5)};
            h.D = {in(t, FE_D), in(t, FE_D + 1)};
            detail::out_f(o, h.second(detail::sym_f(t, SLOT_F), in(t, FE_N)));
        });
        Tracer::cur() = nullptr;
        for (int i = 0; i < 6; ++i) fp.n_slots = std::max(fp.n_slots, fp.all(i)->n_slots);
        return fp;
    }();
    return P;
}
// the 15 constants of the two Frobenius maps in slot order (FE_GAMMA .. FE_NORM + 4), from pairing_k()
inline void final_exp_constants(bls::Fp* out15) {
    const bls::Fp2* g = bls::pairing_k().gamma;
    for (int i = 1; i <= 5; ++i) {
        out15[2 * (i - 1)] = g[i].a;
        out15[2 * (i - 1) + 1] = g[i].b;
        out15[10 + i - 1] = g[i].a.sq() + g[i].b.sq();
    }
}

// The driver: bls::final_exp as a SCHEDULE of four kinds of step over the slots — run a program; copy 12 slots (conjugating or
// not); conjugate F in place; replace FE_N by its inverse unless it is zero.  The schedule is written once, here; the host
// interpreter below and the device kernel k_final_exp (device/pairing.hpp) both walk it, so what the host tests is the order the
// kernel runs.  word: kind | a << 2 | b << 12 | conj << 22
//   t = conj(f) / f ; t = t^(p^2) t ; a = t^x conj(t) ; b = a^x conj(a) ; c = b^x b^p ; d = c^(x^2) conj(c) c^(p^2) ; d t^2 t
enum : uint32_t { FE_RUN = 0, FE_COPY = 1, FE_CONJ = 2, FE_INVERT = 3 };
enum : uint32_t { FE_P_MUL = 0, FE_P_SQ = 1, FE_P_FROB = 2, FE_P_FROB2 = 3, FE_P_INV1 = 4, FE_P_INV2 = 5 };
inline const std::vector<uint32_t>& final_exp_schedule() {
    static const std::vector<uint32_t> sched = [] {
        std::vector<uint32_t> w;
        enum { B0 = FE_BANK, B1 = FE_BANK + 12, B2 = FE_BANK + 24 };
        auto run = [&](uint32_t p) { w.push_back(FE_RUN | p << 2); };
        auto copy = [&](uint32_t dst, uint32_t src, bool conj = false) { w.push_back(FE_COPY | dst << 2 | src << 12 | (conj ? 1u << 22 : 0u)); };
        auto mul_by = [&](uint32_t bank, bool conj = false) {
            copy(SLOT_Y, bank, conj);
            run(FE_P_MUL);
        };
        auto pow_x = [&] {  // F <- F^x (x < 0: the power by |x|, conjugated); the base stays in B1
            copy(B1, SLOT_F);
            for (int b = 62; b >= 0; --b) {
                run(FE_P_SQ);
                if ((0xd201000000010000ull >> b) & 1) mul_by(B1);
            }
            w.push_back(FE_CONJ);
        };
        copy(B0, SLOT_F);
        run(FE_P_INV1);
        w.push_back(FE_INVERT);
        run(FE_P_INV2);
        mul_by(B0, true);        // ^(p^6 - 1)
        copy(B0, SLOT_F);
        run(FE_P_FROB2);
        mul_by(B0);              // ^(p^2 + 1)
        copy(B0, SLOT_F);        // B0 = t from here on
        pow_x();
        mul_by(B1, true);        // a = t^x conj(t)
        pow_x();
        mul_by(B1, true);        // b = a^x conj(a)
        pow_x();                 // b^x, B1 = b
        copy(B2, SLOT_F);
        copy(SLOT_F, B1);
        run(FE_P_FROB);
        mul_by(B2);              // c = b^p b^x
        copy(B2, SLOT_F);        // B2 = c
        pow_x();
        pow_x();                 // c^(x^2)
        mul_by(B2, true);
        copy(B1, SLOT_F);
        copy(SLOT_F, B2);
        run(FE_P_FROB2);
        mul_by(B1);              // d = c^(p^2) c^(x^2) conj(c)
        copy(B1, SLOT_F);
        copy(SLOT_F, B0);
        run(FE_P_SQ);
        mul_by(B0);              // t^3
        mul_by(B1);
        return w;
    }();
    return sched;
}
// the schedule on the host interpreter; sl: the slots with f in F and the constants in place.  false: the norm was zero
inline bool run_final_exp_schedule(const FinalExpPrograms& fp, bls::Fp* sl) {
    for (uint32_t w : final_exp_schedule()) {
        const uint32_t kind = w & 3, a = (w >> 2) & 1023, b = (w >> 12) & 1023, conj = (w >> 22) & 1;
        if (kind == FE_RUN) {
            run_program(*fp.all((int)a), sl);
        } else if (kind == FE_COPY) {
            for (int i = 0; i < 12; ++i) sl[a + i] = conj && i >= 6 ? sl[b + i].neg() : sl[b + i];
        } else if (kind == FE_CONJ) {
            for (int i = 6; i < 12; ++i) sl[SLOT_F + i] = sl[SLOT_F + i].neg();
        } else {
            if (sl[FE_N].is_zero()) return false;
            sl[FE_N] = sl[FE_N].inv();
        }
    }
    return true;
}
// f^(3 (p^12 - 1) / r) through the programs; false for f of norm zero
inline bool final_exp_by_program(const bls::Fp12& f, bls::Fp12& out) {
    static_assert(sizeof(bls::Fp12) == 12 * sizeof(bls::Fp), "Fp12 is 12 packed residues in slot order");
    const FinalExpPrograms& fp = final_exp_programs();
    std::vector<bls::Fp> sl(fp.n_slots, bls::Fp::zero());
    final_exp_constants(&sl[FE_GAMMA]);
    memcpy(&sl[SLOT_F], &f, 12 * sizeof(bls::Fp));
    if (!run_final_exp_schedule(fp, sl.data())) return false;
    memcpy(&out, &sl[SLOT_F], 12 * sizeof(bls::Fp));
    return true;
}

}  // namespace prog
}  // namespace masp_host

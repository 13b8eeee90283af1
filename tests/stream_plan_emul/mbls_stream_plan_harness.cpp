// Host build of the verification stream's round plan and of the one step every walk takes (milagro_bls_amd/csrc/mbls_stream_plan.h, mbls_stream.h), with a plain
// C++ compiler and no HIP. As a shared library for tests/test_stream_plan_cpu.py (sph_*): the plan of a hand-built round, field by field; a whole queue walked
// by stream_walk under the kind's rule, every round planned and measured against meta_capacity. With -DMBLS_STREAM_PLAN_HARNESS_MAIN a program of its own for
// the address and undefined-behaviour sanitizers: every offset table and output array is allocated at exactly its used length, and every data pointer is an
// address nothing is mapped at, so a plan that read a call's data, or an offset table past its end, would abort the program.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../milagro_bls_amd/csrc/mbls_stream_plan.h"

namespace {
struct hpiece { const stream_call* c; uint64_t first, items, round_first, batch; };
stream_round_plan g_plan;

stream_call fake_call(uint64_t j, const mbls_stream_call_shape& sh, bool host, uint32_t bits_len, uint64_t groups) {
    // data "addresses": nothing is mapped there, and array a of call j is told apart from every other
    auto at = [&](uint64_t a) { return (uintptr_t)0x100000000000ull * (a + 1) + (j << 24); };
    stream_call c;
    c.host = host; c.shape = sh; c.bits_len = bits_len; c.groups = groups;
    c.sigs = (const uint8_t*)at(0); c.msgs = (const uint8_t*)at(1); c.keys = (const uint8_t*)at(2); c.bits = bits_len ? (const uint8_t*)at(3) : nullptr;
    c.rands = (const uint64_t*)at(4); c.res = (uint8_t*)at(5); c.bm = (uint64_t*)at(6); c.st = (uint32_t*)at(7); c.set_res = (uint8_t*)at(8); c.set_st = (uint32_t*)at(9);
    return c;
}
}  // namespace

extern "C" {

struct sph_opts { uint32_t kind, verify; uint64_t unit; uint32_t bits_stride, pad; uint64_t round_items, round_keys, round_msg_bytes; };
struct sph_call { uint64_t n; uint32_t k, msg_len; const uint32_t* pk_offsets; const uint64_t* msg_offsets; uint32_t flush_after, host, bits_len, pad; uint64_t groups; };
struct sph_piece { uint64_t call, first, items, round, round_first, batch; };

static stream_consts consts_of(const sph_opts* o) {
    mbls_stream_opts so{}; so.round_items = o->round_items; so.round_keys = o->round_keys; so.round_msg_bytes = o->round_msg_bytes;
    return stream_consts{(int)o->kind, (int)o->verify, o->unit, o->bits_stride, so};
}

uint64_t sph_capacity(const sph_opts* o) { return meta_capacity(consts_of(o)); }
uint64_t sph_tile(int which) { return which == 0 ? GATHER_TILE : which == 1 ? SCATTER_TILE : CMT_TILE; }
// the data address the harness gives array `a` of call j (0 sigs, 1 msgs, 2 keys, 3 bits, 4 rands, 5 res, 6 bm, 7 st, 8 set_res, 9 set_st)
uint64_t sph_addr(uint64_t j, uint64_t a) { return 0x100000000000ull * (a + 1) + (j << 24); }

// the plan of ONE round made of these pieces (piece i: items [first, first + items) of calls[call], at round_first, as batch `batch`); dev: the five device
// arrays of a slot (addresses only). The plan stays in the harness for the getters below.
void sph_plan(const sph_opts* o, const sph_call* calls, uint64_t n_calls, const sph_piece* pieces, uint64_t np, const uint64_t* dev) {
    std::vector<stream_call> cs; std::vector<hpiece> ps;
    for (uint64_t j = 0; j < n_calls; j++)
        cs.push_back(fake_call(j, mbls_stream_call_shape{calls[j].n, calls[j].k, calls[j].msg_len, calls[j].pk_offsets, calls[j].msg_offsets, 0}, calls[j].host != 0, calls[j].bits_len, calls[j].groups));
    for (uint64_t i = 0; i < np; i++) ps.push_back(hpiece{&cs[pieces[i].call], pieces[i].first, pieces[i].items, pieces[i].round_first, pieces[i].batch});
    uint8_t* d[RA_COUNT]; for (int a = 0; a < RA_COUNT; a++) d[a] = (uint8_t*)(uintptr_t)dev[a];
    stream_plan(consts_of(o), ps.data(), ps.size(), d, g_plan);
}
// rows of the last plan as uint64 columns. which: 0 gt {src, dst, bytes}; 1 ct {sigs, midx, cid, bits, bits_len, items, round_first}; 2 vt {sigs, cid, bits, midx,
// rands, bits_len, items, round_first}; 3 st {res, st, bm, call_first, items, round_first}; 4 vst {res, st, set_res, set_st, call_first, items, round_first,
// batch_at}; 5 off32; 6 moff; 7 hc {src, piece, arr, how, len, at, bytes, items}. out = nullptr: the number of rows.
uint64_t sph_rows(int which, uint64_t* out) {
    const stream_round_plan& r = g_plan;
    uint64_t n = 0;
    auto row = [&](std::initializer_list<uint64_t> v) { if (out) for (uint64_t x : v) *out++ = x; n++; };
    switch (which) {
        case 0: for (const gtile& t : r.gt) row({(uintptr_t)t.src, (uintptr_t)t.dst, t.bytes}); break;
        case 1: for (const ctile& t : r.ct) row({(uintptr_t)t.sigs, (uintptr_t)t.midx, (uintptr_t)t.cid, (uintptr_t)t.bits, t.bits_len, t.items, t.round_first}); break;
        case 2: for (const vtile& t : r.vt) row({(uintptr_t)t.sigs, (uintptr_t)t.cid, (uintptr_t)t.bits, (uintptr_t)t.midx, (uintptr_t)t.rands, t.bits_len, t.items, t.round_first}); break;
        case 3: for (const stile& t : r.st) row({(uintptr_t)t.res, (uintptr_t)t.st, (uintptr_t)t.bm, t.call_first, t.items, t.round_first}); break;
        case 4: for (const vstile& t : r.vst) row({(uintptr_t)t.res, (uintptr_t)t.st, (uintptr_t)t.set_res, (uintptr_t)t.set_st, t.call_first, t.items, t.round_first, t.batch_at}); break;
        case 5: for (uint32_t v : r.off32) row({v}); break;
        case 6: for (uint64_t v : r.moff) row({v}); break;
        default: for (const stream_hcopy& c : r.hc) row({(uintptr_t)c.src, c.piece, c.arr, c.how, c.len, c.at, c.bytes, c.items}); break;
    }
    return n;
}
// {keys_uniform, msgs_uniform, k, msg_len, n, batches, max_groups, gathered, any_host, at_g, at_s, at_k, at_m, at_c, bytes}
void sph_scalars(uint64_t* out) {
    const stream_round_plan& r = g_plan;
    const uint64_t v[15] = {(uint64_t)r.lay.keys_uniform, (uint64_t)r.lay.msgs_uniform, r.lay.k, r.lay.msg_len, r.n, r.batches, r.max_groups, r.gathered, r.any_host,
                            r.at_g, r.at_s, r.at_k, r.at_m, r.at_c, r.bytes};
    memcpy(out, v, sizeof(v));
}
// the last plan's meta area, exactly `bytes` of the scalars
void sph_pack(uint8_t* meta) { stream_plan_pack(g_plan, meta); }

// fields of len bytes -> fields of stride bytes (stream_widen, the one function both staging strategies use)
void sph_widen(uint8_t* dst, const uint8_t* src, uint64_t items, uint32_t len, uint64_t stride) { stream_widen(dst, src, items, len, stride); }

// A whole queue walked by stream_walk under the kind's rule (calls[j].flush_after closes the round behind call j): every piece it makes -> out[0 .. *n_pieces)
// (as many as max_pieces hold), and for every round r the plan of its pieces -> info[4 r ..] = {the plan's meta bytes, what of round_items the round uses
// (stream_vm_used on a stream of whole calls), its items, its whole calls}. Returns the rounds, -1 if a call joins no empty round, -2 for more than max_rounds.
int64_t sph_walk(const sph_opts* o, const sph_call* calls, uint64_t n_calls, sph_piece* out, uint64_t max_pieces, uint64_t* n_pieces, uint64_t* info, uint64_t max_rounds) {
    const stream_consts k = consts_of(o);
    const int whole = stream_kind_whole(k.kind);
    std::vector<stream_call> cs;
    for (uint64_t j = 0; j < n_calls; j++)
        cs.push_back(fake_call(j, mbls_stream_call_shape{calls[j].n, calls[j].k, calls[j].msg_len, calls[j].pk_offsets, calls[j].msg_offsets, calls[j].flush_after}, calls[j].host != 0,
                               calls[j].bits_len, calls[j].groups));
    std::vector<hpiece> ps; uint64_t np = 0, cur = 0; bool over = false; mbls_stream_fill last{};
    uint8_t* d[RA_COUNT]; for (int a = 0; a < RA_COUNT; a++) d[a] = (uint8_t*)(uintptr_t)sph_addr(1000000 + a, 0);
    stream_round_plan plan;
    auto close = [&]() {
        if (ps.empty()) return;
        if (cur >= max_rounds) { over = true; ps.clear(); return; }
        stream_plan(k, ps.data(), ps.size(), d, plan);
        info[4 * cur] = plan.bytes; info[4 * cur + 1] = whole ? stream_vm_used(last) : last.items; info[4 * cur + 2] = last.items; info[4 * cur + 3] = last.calls;
        ps.clear();
    };
    const int64_t rounds = stream_walk(k.o, whole, n_calls, [&](uint64_t j) { return cs[j].shape; },
        [&](uint64_t j, uint64_t first, const mbls_stream_step& st, uint64_t round, const mbls_stream_fill& f) {
            if (round != cur) { close(); cur = round; }
            ps.push_back(hpiece{&cs[j], first, st.items, st.round_first, st.batch});
            last = f;
            if (np < max_pieces) out[np] = sph_piece{j, first, st.items, round, st.round_first, st.batch};
            np++;
        });
    close();
    *n_pieces = np;
    return rounds < 0 ? -1 : over ? -2 : rounds;
}

}  // extern "C"

#ifdef MBLS_STREAM_PLAN_HARNESS_MAIN
// random queues of every kind, every array at exactly its used length
int main() {
    unsigned long checked = 0;
    uint32_t seed = 777;
    auto next = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (int trial = 0; trial < 300; trial++) {
        sph_opts o{}; o.kind = trial % 3; o.verify = 0; o.bits_stride = 20;
        o.round_items = 2 + next() % 600; o.round_keys = 1 + next() % (4 * o.round_items); o.round_msg_bytes = 4 * o.round_items + next() % 64;
        o.unit = o.kind == STREAM_KEYS ? (trial & 1 ? 48 : 4) : 0;
        const uint64_t n_calls = 1 + next() % 24;
        sph_call* calls = (sph_call*)malloc(sizeof(sph_call) * n_calls);
        uint64_t items = 0;
        for (uint64_t j = 0; j < n_calls; j++) {
            sph_call& c = calls[j]; memset(&c, 0, sizeof(c));
            c.n = 1 + next() % (o.kind == STREAM_VM ? o.round_items - 1 : 2 * o.round_items);
            c.host = next() % 3 == 0; c.flush_after = next() % 7 == 0; c.groups = c.n;
            c.bits_len = o.kind == STREAM_KEYS ? 0 : o.kind == STREAM_VM ? next() % 21 : 1 + next() % 20;
            c.msg_len = 4;
            if (o.kind == STREAM_KEYS) {
                c.k = next() % 2; c.msg_len = next() % 5;
                if (next() % 2) { uint32_t* t = (uint32_t*)malloc(4 * (c.n + 1)); t[0] = next() % 9; for (uint64_t i = 0; i < c.n; i++) t[i + 1] = t[i] + next() % 2; c.pk_offsets = t; }
                if (next() % 2) { uint64_t* t = (uint64_t*)malloc(8 * (c.n + 1)); t[0] = next() % 9; for (uint64_t i = 0; i < c.n; i++) t[i + 1] = t[i] + next() % 5; c.msg_offsets = t; }
            }
            items += c.n;
        }
        const uint64_t max_pieces = items, max_rounds = items;      // a piece and a round hold at least one item
        sph_piece* out = (sph_piece*)malloc(sizeof(sph_piece) * max_pieces);
        uint64_t* info = (uint64_t*)malloc(32 * max_rounds);
        uint64_t np = 0;
        const int64_t rounds = sph_walk(&o, calls, n_calls, out, max_pieces, &np, info, max_rounds);
        if (rounds < 1 || np > max_pieces) { printf("FAIL walk %d -> %lld\n", trial, (long long)rounds); return 1; }
        const uint64_t cap = sph_capacity(&o);
        for (int64_t r = 0; r < rounds; r++) {
            if (info[4 * r] > cap || info[4 * r + 1] > o.round_items) { printf("FAIL round %d/%lld: %llu bytes of %llu\n", trial, (long long)r, (unsigned long long)info[4 * r], (unsigned long long)cap); return 1; }
            checked++;
        }
        // the last round once more through the single-round entry, packed into a block of exactly its bytes
        uint64_t a = np; while (a > 0 && out[a - 1].round == (uint64_t)rounds - 1) a--;
        const uint64_t dev[5] = {sph_addr(9000, 0), sph_addr(9001, 0), sph_addr(9002, 0), sph_addr(9003, 0), sph_addr(9004, 0)};
        sph_plan(&o, calls, n_calls, out + a, np - a, dev);
        uint64_t sc[15]; sph_scalars(sc);
        if (sc[14] != info[4 * (rounds - 1)]) { printf("FAIL replan %d\n", trial); return 1; }
        uint8_t* meta = (uint8_t*)malloc(sc[14] ? sc[14] : 1);
        sph_pack(meta);
        free(meta); free(info); free(out);
        for (uint64_t j = 0; j < n_calls; j++) { free((void*)calls[j].pk_offsets); free((void*)calls[j].msg_offsets); }
        free(calls);
    }
    // widening: source fields end with their block, the destination is exactly items x stride
    for (uint32_t len : {0u, 1u, 19u, 20u})
        for (uint64_t items = 1; items <= 3; items++) {
            uint8_t* src = len ? (uint8_t*)malloc(len * items) : nullptr; uint8_t* dst = (uint8_t*)malloc(20 * items);
            for (uint64_t b = 0; b < len * items; b++) src[b] = (uint8_t)next() | 1;
            memset(dst, 0xA5, 20 * items);
            sph_widen(dst, src, items, len, 20);
            for (uint64_t i = 0; i < items; i++)
                for (uint32_t b = 0; b < 20; b++) { if (dst[20 * i + b] != (b < len ? src[len * i + b] : 0)) { printf("FAIL widen %u\n", len); return 1; } checked++; }
            free(src); free(dst);
        }
    printf("ok %lu checks\n", checked);
    return 0;
}
#endif

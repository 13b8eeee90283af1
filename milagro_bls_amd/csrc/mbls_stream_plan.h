// mbls_stream_plan.h -- what a round of the verification stream looks like, as pure host code (no HIP: tests/stream_plan_emul/mbls_stream_plan_harness.cpp builds
// it with a plain C++ compiler): the kinds of stream, the tile records the five stream kernels read, and one PLAN function per kind. From the round's pieces and
// the stream's constants a plan gives the tile lists, the host copies in the order they are issued, the offset tables (or the batch table), the layout decision,
// the statistic `gathered`, and where each part lies in the slot's meta area. It reads the calls' host-side offset tables and never their data: every data
// pointer is only offset and stored. launch_round (mbls_stream.hip) makes the plan and issues it; meta_capacity, below the plans, bounds what they can need.
#ifndef MBLS_STREAM_PLAN_H
#define MBLS_STREAM_PLAN_H
#include <string.h>
#include <vector>
#include "mbls_stream.h"

// a stream's kind, fixed at creation: what a call's arrays are, whether a call may be split, which slot buffers exist, which entry a round calls, how a host
// piece is staged and how answers go back all follow from it (mbls_stream.hip: one switch per function)
enum stream_kind {
    STREAM_KEYS = 0,         // signatures, messages (bytes, or indices into a message table) and keys (bytes, or indices into a key table); calls may be split
    STREAM_COMMITTEE = 1,    // signatures, message indices, committee ids and bitfields of bits_len bytes; calls may be split
    STREAM_VM = 2            // whole verify_multiple batches over the same arrays plus blinding scalars; a call is never split and is one batch of its round
};
static inline int stream_kind_whole(int kind) { return kind == STREAM_VM; }
struct stream_consts { int kind; int verify; uint64_t unit; uint32_t bits_stride; mbls_stream_opts o; };   // verify: one key per item (MBLS_STREAM_VERIFY)

namespace {   // (unnamed to the end of the header, like the host side of mbls_stream.hip: the kernels' parameter types are spelled in their names)

constexpr uint64_t GATHER_TILE = 128 * 1024;         // bytes per gather tile (a multiple of 16: tiles of one segment keep its alignment)
constexpr uint64_t SCATTER_TILE = 4096;              // items per scatter tile, cut at multiples of this in the CALL's item space (so at bitmap words)
constexpr uint64_t CMT_TILE = 256;                   // items per gather tile of a committee piece

struct gtile { const uint8_t* src; uint8_t* dst; uint64_t bytes; };
struct stile { uint8_t* res; uint32_t* st; uint64_t* bm; uint64_t call_first, items, round_first; };
// a tile of a committee piece: the caller's four arrays at the tile's first item, and where its items lie in the round
struct ctile { const uint8_t* sigs; const uint32_t* midx; const uint32_t* cid; const uint8_t* bits; uint32_t bits_len, items; uint64_t round_first; };
// a tile of at most CMT_TILE sets of a verify_multiple call: the caller's five arrays at the tile's first set, and where its sets lie in the round
struct vtile { const uint8_t* sigs; const uint32_t* cid; const uint8_t* bits; const uint32_t* midx; const uint64_t* rands; uint32_t bits_len, items; uint64_t round_first; };
// a device call's outputs: sets [call_first, call_first + items) of the call are sets [round_first, ...) of the round; the tile at call_first = 0 also carries the
// call's batch byte and word, which the round keeps at n_round + batch
struct vstile { uint8_t* res; uint32_t* st; uint8_t* set_res; uint32_t* set_st; uint64_t call_first, items, round_first, batch_at; };
static_assert(sizeof(gtile) == 24 && sizeof(stile) == 48 && sizeof(ctile) == 48 && sizeof(vtile) == 56 && sizeof(vstile) == 64, "the kernels read these records");

// what the launcher knows of a submitted call. keys: key bytes or indices (a committee or verify_multiple call: its committee ids); msgs: message bytes or
// indices; bits: bits_len bytes per item; a verify_multiple call (shape.n sets; res / st: ONE byte and word) also has its scalars, its per-set outputs and the
// groups it may form
struct stream_call {
    bool host = false; mbls_stream_call_shape shape{};
    const uint8_t* sigs = nullptr; const uint8_t* msgs = nullptr; const uint8_t* keys = nullptr; const uint8_t* bits = nullptr; uint32_t bits_len = 0;
    uint8_t* res = nullptr; uint64_t* bm = nullptr; uint32_t* st = nullptr;
    const uint64_t* rands = nullptr; uint8_t* set_res = nullptr; uint32_t* set_st = nullptr; uint64_t groups = 0;
};

// the arrays of a round, as the slot holds them on the device (and, where a kind stages through pinned memory, in a pinned mirror)
enum stream_array { RA_SIGS = 0, RA_MSGS, RA_KEYS /* key bytes or indices; the bitfields at the stream's stride */, RA_CID, RA_RANDS, RA_COUNT };

// one step of bringing a host piece's bytes into the round, in the order the steps are taken. `piece`: the step is taken when the issue loop reaches that piece
// (before the wait on its event, if it has one; pieces.size(): behind the last piece). DIRECT: an upload of `bytes` from the caller's memory at src to array
// `arr` at byte `at`. STAGE: a memcpy of the same bytes into the pinned mirror of the array; WIDEN: `items` bitfields of `len` bytes at src, each widened to
// bytes / items in the mirror (stream_widen); UPLOAD: `bytes` of the mirror at `at` to the array at `at`.
enum stream_hcopy_how { HC_DIRECT = 0, HC_STAGE, HC_WIDEN, HC_UPLOAD };
struct stream_hcopy { const uint8_t* src; uint32_t piece, arr, how, len; uint64_t at, bytes, items; };

// fields of len bytes back to back at src -> fields of stride >= len bytes at dst, every byte beyond len zero (len = 0: nothing is read)
static inline void stream_widen(uint8_t* dst, const uint8_t* src, uint64_t items, uint32_t len, uint64_t stride) {
    if (len == stride) { if (stride) memcpy(dst, src, stride * items); return; }
    for (uint64_t i = 0; i < items; i++) {
        if (len) memcpy(dst + stride * i, src + (uint64_t)len * i, len);
        memset(dst + stride * i + len, 0, stride - len);
    }
}

// the plan of one round. Vectors a kind does not use stay empty; a slot keeps its plan, so a round allocates nothing once the vectors have grown.
struct stream_round_plan {
    std::vector<gtile> gt; std::vector<ctile> ct; std::vector<vtile> vt;     // gather tiles: byte segments (keys), committee pieces, verify_multiple calls
    std::vector<stile> st; std::vector<vstile> vst;                           // scatter tiles of the device pieces
    std::vector<uint32_t> off32;                                              // keys: the round's key offsets, n + 1, where keys are ragged; verify_multiple: the batch table, batches + 1
    std::vector<uint64_t> moff;                                               // keys: the round's message offsets, n + 1, where messages are ragged
    std::vector<uint64_t> sets;                                               // verify_multiple: the sets of each batch
    std::vector<stream_hcopy> hc;
    mbls_stream_layout lay;
    uint64_t n, batches, max_groups, gathered; bool any_host;                 // n: items (sets) of the round; batches, max_groups: verify_multiple
    // the meta area: gather tiles (gt or vt) at at_g | scatter tiles at at_s | off32 at at_k | moff at at_m | ct at at_c; bytes: its end
    uint64_t at_g, at_s, at_k, at_m, at_c, bytes;
    void clear() {
        gt.clear(); ct.clear(); vt.clear(); st.clear(); vst.clear(); off32.clear(); moff.clear(); sets.clear(); hc.clear();
        lay = mbls_stream_layout{1, 1, 0, 0}; n = batches = max_groups = gathered = 0; any_host = false; at_g = at_s = at_k = at_m = at_c = bytes = 0;
    }
};

static inline uint64_t stream_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

static inline void stream_plan_hcopy(stream_round_plan& r, uint32_t how, size_t piece, const void* src, uint32_t arr, uint64_t at, uint64_t bytes, uint32_t len = 0, uint64_t items = 0) {
    if (bytes) r.hc.push_back(stream_hcopy{(const uint8_t*)src, (uint32_t)piece, arr, how, len, at, bytes, items});
}
// the scatter tiles of a device piece of a keys or committee call: cut at multiples of SCATTER_TILE in the call's item space
template <typename P>
static inline void stream_plan_scatter(stream_round_plan& r, const P& p) {
    for (uint64_t a = p.first; a < p.first + p.items;) {
        const uint64_t b = p.first + p.items < (a / SCATTER_TILE + 1) * SCATTER_TILE ? p.first + p.items : (a / SCATTER_TILE + 1) * SCATTER_TILE;
        r.st.push_back(stile{p.c->res, p.c->st, p.c->bm, a, b - a, p.round_first + (a - p.first)});
        a = b;
    }
}
// the meta area of a keys or committee round
static inline void stream_plan_meta(stream_round_plan& r) {
    r.at_g = 0; r.at_s = stream_up(r.at_g + r.gt.size() * sizeof(gtile), 16); r.at_k = stream_up(r.at_s + r.st.size() * sizeof(stile), 8);
    r.at_m = stream_up(r.at_k + r.off32.size() * 4, 8); r.at_c = stream_up(r.at_m + r.moff.size() * 8, 16); r.bytes = r.at_c + r.ct.size() * sizeof(ctile);
}

// A keys round. Every piece brings three byte segments -- signatures, messages, keys (`unit` bytes each) -- to the next free place of the round's arrays
// (dev[RA_*]: the slot's device arrays, only offset): a host piece by one DIRECT copy per non-empty segment, a device piece by one gather tile per GATHER_TILE bytes.
// The layout is uniform where every piece shares it (verify: one key per item whatever the shapes say); otherwise the round's offset tables are built from the calls'.
template <typename P>
static inline void stream_plan_keys(const stream_consts& k, const P* pieces, size_t np, uint8_t* const* dev, stream_round_plan& r) {
    r.clear();
    for (size_t i = 0; i < np; i++) { stream_layout_add(r.lay, i == 0, pieces[i].c->shape); r.n += pieces[i].items; }
    if (k.verify) { r.lay.keys_uniform = 1; r.lay.k = 1; }
    if (!r.lay.keys_uniform) r.off32.resize(r.n + 1);
    if (!r.lay.msgs_uniform) r.moff.resize(r.n + 1);
    uint64_t key_cur = 0, msg_cur = 0;
    for (size_t i = 0; i < np; i++) {
        const P& p = pieces[i]; const stream_call& c = *p.c; const mbls_stream_call_shape& sh = c.shape;
        r.any_host |= c.host;
        auto seg = [&](const uint8_t* src, uint32_t arr, uint64_t at, uint64_t bytes) {
            r.gathered += bytes;
            if (c.host) { stream_plan_hcopy(r, HC_DIRECT, i, src, arr, at, bytes); return; }
            for (uint64_t o = 0; o < bytes; o += GATHER_TILE) r.gt.push_back(gtile{src + o, dev[arr] + at + o, GATHER_TILE < bytes - o ? GATHER_TILE : bytes - o});
        };
        seg(c.sigs + 96 * p.first, RA_SIGS, 96 * p.round_first, 96 * p.items);
        const uint64_t m0 = sh.msg_offsets ? sh.msg_offsets[p.first] : (uint64_t)sh.msg_len * p.first;
        const uint64_t mb = sh.msg_offsets ? sh.msg_offsets[p.first + p.items] - m0 : (uint64_t)sh.msg_len * p.items;
        seg(c.msgs + m0, RA_MSGS, msg_cur, mb);
        const uint64_t k0 = sh.pk_offsets ? sh.pk_offsets[p.first] : (uint64_t)sh.k * p.first;
        const uint64_t kc = sh.pk_offsets ? sh.pk_offsets[p.first + p.items] - k0 : (uint64_t)sh.k * p.items;
        seg(c.keys + k.unit * k0, RA_KEYS, k.unit * key_cur, k.unit * kc);
        if (!r.lay.keys_uniform || !r.lay.msgs_uniform)
            for (uint64_t j = 0; j < p.items; j++) {
                if (!r.lay.keys_uniform) r.off32[p.round_first + j] = (uint32_t)(key_cur + (sh.pk_offsets ? sh.pk_offsets[p.first + j] - k0 : (uint64_t)sh.k * j));
                if (!r.lay.msgs_uniform) r.moff[p.round_first + j] = msg_cur + (sh.msg_offsets ? sh.msg_offsets[p.first + j] - m0 : (uint64_t)sh.msg_len * j);
            }
        key_cur += kc; msg_cur += mb;
        if (!c.host) stream_plan_scatter(r, p);
    }
    if (!r.lay.keys_uniform) r.off32[r.n] = (uint32_t)key_cur;
    if (!r.lay.msgs_uniform) r.moff[r.n] = msg_cur;
    stream_plan_meta(r);
}

// A committee round: the four arrays dense in round order, every field at the stream's stride. A device piece is one record per CMT_TILE items (k_stream_gather_cmt
// copies three arrays and re-strides the fields). A host piece is three DIRECT copies from the caller's memory; only its fields go through pinned memory, widened
// to the stride. `gathered` counts the bytes the call carries.
template <typename P>
static inline void stream_plan_committee(const stream_consts& k, const P* pieces, size_t np, stream_round_plan& r) {
    r.clear();
    const uint64_t bs = k.bits_stride;
    for (size_t i = 0; i < np; i++) {
        const P& p = pieces[i]; const stream_call& c = *p.c;
        r.n += p.items; r.any_host |= c.host;
        r.gathered += (96 + 4 + 4 + (uint64_t)c.bits_len) * p.items;
        const uint8_t* bits = c.bits + (uint64_t)c.bits_len * p.first;
        if (c.host) {
            stream_plan_hcopy(r, HC_DIRECT, i, c.sigs + 96 * p.first, RA_SIGS, 96 * p.round_first, 96 * p.items);
            stream_plan_hcopy(r, HC_DIRECT, i, c.msgs + 4 * p.first, RA_MSGS, 4 * p.round_first, 4 * p.items);
            stream_plan_hcopy(r, HC_DIRECT, i, c.keys + 4 * p.first, RA_CID, 4 * p.round_first, 4 * p.items);
            stream_plan_hcopy(r, HC_WIDEN, i, bits, RA_KEYS, bs * p.round_first, bs * p.items, c.bits_len, p.items);
            stream_plan_hcopy(r, HC_UPLOAD, i, nullptr, RA_KEYS, bs * p.round_first, bs * p.items);
            continue;
        }
        const uint32_t* midx = (const uint32_t*)c.msgs; const uint32_t* cid = (const uint32_t*)c.keys;
        for (uint64_t a = p.first; a < p.first + p.items; a += CMT_TILE)
            r.ct.push_back(ctile{c.sigs + 96 * a, midx + a, cid + a, c.bits + (uint64_t)c.bits_len * a, c.bits_len,
                                 (uint32_t)(CMT_TILE < p.first + p.items - a ? CMT_TILE : p.first + p.items - a), p.round_first + (a - p.first)});
        stream_plan_scatter(r, p);
    }
    stream_plan_meta(r);
}

// A verify_multiple round: every piece is a whole call and batch p.batch of the round; the round keeps the sets' bytes and words at [0, n) of its result arrays
// and the batches' behind them at [n, n + batches). A device call is one gather record per CMT_TILE sets and one scatter record per SCATTER_TILE sets. Host calls
// are laid into the pinned mirrors at their sets' places (STAGE, the fields WIDEN), and every RUN of neighbouring host calls goes up in five UPLOADs when the run
// ends -- a round of small host calls would otherwise pay five pageable copies per call. The batch table is stream_vm_offsets of the calls' sets.
template <typename P>
static inline void stream_plan_vm(const stream_consts& k, const P* pieces, size_t np, stream_round_plan& r) {
    r.clear();
    const uint64_t bs = k.bits_stride;
    for (size_t i = 0; i < np; i++) r.n += pieces[i].items;
    r.batches = np; r.sets.resize(np); r.off32.resize(np + 1);
    uint64_t run_lo = 0, run_hi = 0;
    auto flush_run = [&](size_t at_piece) {
        const uint64_t a = run_lo, m = run_hi - run_lo;
        if (!m) return;
        stream_plan_hcopy(r, HC_UPLOAD, at_piece, nullptr, RA_SIGS, 96 * a, 96 * m); stream_plan_hcopy(r, HC_UPLOAD, at_piece, nullptr, RA_CID, 4 * a, 4 * m);
        stream_plan_hcopy(r, HC_UPLOAD, at_piece, nullptr, RA_MSGS, 4 * a, 4 * m); stream_plan_hcopy(r, HC_UPLOAD, at_piece, nullptr, RA_RANDS, 8 * a, 8 * m);
        stream_plan_hcopy(r, HC_UPLOAD, at_piece, nullptr, RA_KEYS, bs * a, bs * m);
        run_lo = run_hi = 0;
    };
    for (size_t i = 0; i < np; i++) {
        const P& p = pieces[i]; const stream_call& c = *p.c; const uint64_t m = p.items, r0 = p.round_first;
        r.sets[p.batch] = m; r.max_groups += c.groups;
        r.gathered += (96 + 4 + 4 + 8 + (uint64_t)c.bits_len) * m;
        if (c.host) {
            r.any_host = true;
            if (run_hi != r0) { flush_run(i); run_lo = r0; }
            run_hi = r0 + m;
            stream_plan_hcopy(r, HC_STAGE, i, c.sigs, RA_SIGS, 96 * r0, 96 * m); stream_plan_hcopy(r, HC_STAGE, i, c.keys, RA_CID, 4 * r0, 4 * m);
            stream_plan_hcopy(r, HC_STAGE, i, c.msgs, RA_MSGS, 4 * r0, 4 * m); stream_plan_hcopy(r, HC_STAGE, i, c.rands, RA_RANDS, 8 * r0, 8 * m);
            stream_plan_hcopy(r, HC_WIDEN, i, c.bits, RA_KEYS, bs * r0, bs * m, c.bits_len, m);
            continue;
        }
        flush_run(i);
        const uint32_t* cid = (const uint32_t*)c.keys; const uint32_t* midx = (const uint32_t*)c.msgs;
        for (uint64_t a = 0; a < m; a += CMT_TILE)
            r.vt.push_back(vtile{c.sigs + 96 * a, cid + a, c.bits_len ? c.bits + (uint64_t)c.bits_len * a : nullptr, midx + a, c.rands + a, c.bits_len,
                                 (uint32_t)(CMT_TILE < m - a ? CMT_TILE : m - a), r0 + a});
        for (uint64_t a = 0; a < m; a += SCATTER_TILE)
            r.vst.push_back(vstile{c.res, c.st, c.set_res, c.set_st, a, SCATTER_TILE < m - a ? SCATTER_TILE : m - a, r0 + a, r.n + p.batch});
    }
    flush_run(np);
    stream_vm_offsets(r.sets.data(), r.batches, r.off32.data());
    r.at_g = 0; r.at_s = stream_up(r.at_g + r.vt.size() * sizeof(vtile), 16); r.at_k = stream_up(r.at_s + r.vst.size() * sizeof(vstile), 16);
    r.at_m = r.at_c = r.bytes = r.at_k + 4 * (r.batches + 1);
}

template <typename P>
static inline void stream_plan(const stream_consts& k, const P* pieces, size_t np, uint8_t* const* dev, stream_round_plan& r) {
    switch (k.kind) {
        case STREAM_KEYS: stream_plan_keys(k, pieces, np, dev, r); break;
        case STREAM_COMMITTEE: stream_plan_committee(k, pieces, np, r); break;
        default: stream_plan_vm(k, pieces, np, r); break;
    }
}

// the plan's records and tables into the (pinned) meta area, r.bytes of it
static inline void stream_plan_pack(const stream_round_plan& r, uint8_t* meta) {
    auto put = [&](uint64_t at, const void* src, size_t bytes) { if (bytes) memcpy(meta + at, src, bytes); };
    put(r.at_g, r.gt.data(), r.gt.size() * sizeof(gtile)); put(r.at_g, r.vt.data(), r.vt.size() * sizeof(vtile));
    put(r.at_s, r.st.data(), r.st.size() * sizeof(stile)); put(r.at_s, r.vst.data(), r.vst.size() * sizeof(vstile));
    put(r.at_k, r.off32.data(), r.off32.size() * 4); put(r.at_m, r.moff.data(), r.moff.size() * 8); put(r.at_c, r.ct.data(), r.ct.size() * sizeof(ctile));
}

// The most meta bytes a plan of this kind can need, whatever the cutting rule puts into a round of R = round_items (tests/test_stream_plan_cpu.py holds every
// plan against it). Keys and committee: a round has at most R pieces. A segment of b bytes takes at most b / GATHER_TILE + 1 gather tiles and a piece has three; a
// piece of m items takes at most m / SCATTER_TILE + 2 scatter tiles (it may straddle a tile boundary of its call) and at most m / CMT_TILE + 1 committee tiles;
// both offset tables hold R + 1 entries. Verify_multiple: at most R / 2 calls (the smallest costs 2), each of m sets at most m / tile + 1 gather and as many
// scatter tiles, and the batch table. 64 bytes cover the alignment of the parts.
static inline uint64_t meta_capacity(const stream_consts& c) {
    const uint64_t R = c.o.round_items;
    if (c.kind == STREAM_VM) return (R + R / CMT_TILE + 1) * sizeof(vtile) + (R + R / SCATTER_TILE + 1) * sizeof(vstile) + 4 * (R + 2) + 64;
    const uint64_t bytes = 96 * R + c.o.round_msg_bytes + c.unit * c.o.round_keys;
    const uint64_t ng = bytes / GATHER_TILE + 3 * R + 3, ns = 2 * R + R / SCATTER_TILE + 1;
    const uint64_t nc = c.kind == STREAM_COMMITTEE ? R + R / CMT_TILE + 1 : 0;
    return ng * sizeof(gtile) + ns * sizeof(stile) + nc * sizeof(ctile) + 4 * (R + 1) + 8 * (R + 1) + 64;
}

}  // namespace
#endif

// mbls_stream.hip -- the verification stream (include/mbls.h, "verification stream"): calls of any size in, full-round launches of the
// public device entries out. Built on the public ABI only: mbls_ctx_get_limits, mbls_ctx_reserve[_keys], mbls_plan_workspace_items and the
// three *_device verification entries (a message-table stream: their `_msgtable_device` forms), so every result comes out of the same verify_pipeline the parity
// tests pin. One hook below the ABI, not exported from the library: a message table counts the calls its streams hold (mblsi_msgtable_stream_calls), which mbls_msgtable_clear consults.
// A committee stream (mbls_stream_create_committee) launches mbls_fast_aggregate_verify_batch_committee_msgtable_device over the slot; its device pieces are staged
// by k_stream_gather_cmt, which re-strides every call's bitfields to the stream's stride, and its table is held by two more such hooks (mblsi_committees_stream_*).
// A verify_multiple stream (mbls_stream_create_vm_committee) takes whole batches: a call is never split (stream_take_whole, the rule mbls_stream_cut_vm states as
// data), a round is ONE call of mbls_verify_multiple_batches_committee_msgtable_locate_device over the slot with a ragged batch table the launcher builds, staged
// by k_stream_gather_vm and answered per call and per set by k_stream_scatter_vm; one more hook reserves that entry's own staging (mblsi_vbg_reserve_staging).
//
// Per stream: depth + 1 staging SLOTS (one round each: the open one and up to depth launched), one LAUNCHER thread that cuts the queue of
// submitted calls into the open slot (stream_take, the rule mbls_stream_cut states as data), gathers the round's inputs into the slot on the
// stream's gather stream (k_stream_gather; host pieces by hipMemcpyAsync), runs the device entry on the stream's main HIP stream, scatters
// the results back to the callers (k_stream_scatter; host pieces through a pinned area) and records a blocking-sync event, and one COMPLETER
// thread that waits on those events in order, copies host results, advances completed_through and frees the slot. Neither thread calls into
// the context with the stream's lock held; no HIP call is made from a host callback.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>
#include "mbls_stream.h"

// the table's count of calls that streams bound to it have taken and not completed (mbls_kernels.hip; mbls_msgtable_clear refuses while there are any)
extern "C" __attribute__((visibility("hidden"))) void mblsi_msgtable_stream_calls(mbls_msgtable* t, long long delta);
// a committee stream's two interlocks with its table (mbls_kernels.hip): the same count, which mbls_committees_clear consults, and the binding of the stream's
// bits_stride, which checks the table against the stream's context and stride and from then on keeps mbls_committees_append inside it
extern "C" __attribute__((visibility("hidden"))) void mblsi_committees_stream_calls(mbls_committees* t, long long delta);
extern "C" __attribute__((visibility("hidden"))) int mblsi_committees_stream_bind(mbls_ctx* ctx, mbls_committees* t, uint32_t bits_stride);
extern "C" __attribute__((visibility("hidden"))) void mblsi_committees_stream_unbind(mbls_committees* t, uint32_t bits_stride);
// a verify_multiple stream: the staging mbls_verify_multiple_batches_committee_msgtable* takes beside the workspace and the committee scratch (mbls_kernels.hip: the
// set map of a ragged batch table, the group arrays), which has no public reserve
extern "C" __attribute__((visibility("hidden"))) int mblsi_vbg_reserve_staging(mbls_ctx* ctx, uint64_t max_sets, uint64_t max_batches);

namespace {

constexpr unsigned SWG = 64;                        // one wave per workgroup, like the rest of the library
constexpr uint64_t GATHER_TILE = 128 * 1024;         // bytes per gather tile (a multiple of 16: tiles of one segment keep its alignment)
constexpr uint64_t SCATTER_TILE = 4096;              // items per scatter tile, cut at multiples of this in the CALL's item space (so at bitmap words)
constexpr uint64_t CMT_TILE = 256;                   // items per gather tile of a committee piece

struct gtile { const uint8_t* src; uint8_t* dst; uint64_t bytes; };
struct stile { uint8_t* res; uint32_t* st; uint64_t* bm; uint64_t call_first, items, round_first; };
// a tile of a committee piece: the caller's four arrays at the tile's first item, and where its items lie in the round
struct ctile { const uint8_t* sigs; const uint32_t* midx; const uint32_t* cid; const uint8_t* bits; uint32_t bits_len, items; uint64_t round_first; };

// the wave's copy of one segment: 16-byte loads and stores where source and destination are both 16-byte aligned, dwords where both are 4-byte aligned, bytes
// otherwise (ragged messages start anywhere)
__device__ __forceinline__ void wave_copy(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint64_t bytes, unsigned l) {
    const uintptr_t a = (uintptr_t)src | (uintptr_t)dst;
    uint64_t done = 0;
    if ((a & 15) == 0) {
        const uint64_t n16 = bytes / 16;
        const uint4* s = (const uint4*)src; uint4* d = (uint4*)dst;
#pragma unroll 4
        for (uint64_t i = l; i < n16; i += SWG) d[i] = s[i];
        done = 16 * n16;
    } else if ((a & 3) == 0) {
        const uint64_t n4 = bytes / 4;
        const uint32_t* s = (const uint32_t*)src; uint32_t* d = (uint32_t*)dst;
#pragma unroll 4
        for (uint64_t i = l; i < n4; i += SWG) d[i] = s[i];
        done = 4 * n4;
    }
    for (uint64_t i = done + l; i < bytes; i += SWG) dst[i] = src[i];
}

// every destination dword of a tile's fields, lanes over consecutive dwords (T: the width the dword count fits)
template <typename T>
__device__ __forceinline__ void wave_restride(const ctile& t, uint32_t* __restrict__ dst, uint32_t dwords_per_item, int fast, unsigned l) {
    const T nd = (T)t.items * dwords_per_item;
    for (T w = l; w < nd; w += SWG) {
        const T i = w / dwords_per_item;
        dst[w] = stream_bits_dword(t.bits + (uint64_t)t.bits_len * i, t.bits_len, (uint32_t)(w - i * dwords_per_item), fast);
    }
}

}  // namespace

// One workgroup per tile (wave_copy).
__global__ __launch_bounds__(SWG) void k_stream_gather(const gtile* __restrict__ tiles) {
    const gtile t = tiles[blockIdx.x];
    wave_copy(t.src, t.dst, t.bytes, threadIdx.x);
}

// One workgroup per tile of at most CMT_TILE items of a committee piece: signatures, message indices and committee ids copied to the round's arrays at
// round_first (wave_copy), the bitfields re-strided from bits_len bytes at any address to the slot's bits_stride (stream_bits_dword: every dword of every
// item's stride is written, so a slot never shows a round the bits of the round before).
__global__ __launch_bounds__(SWG) void k_stream_gather_cmt(const ctile* __restrict__ tiles, uint8_t* __restrict__ d_sigs, uint32_t* __restrict__ d_midx,
                                                           uint32_t* __restrict__ d_cid, uint8_t* __restrict__ d_bits, uint32_t bits_stride) {
    const ctile t = tiles[blockIdx.x];
    const unsigned l = threadIdx.x;
    wave_copy(t.sigs, d_sigs + 96 * t.round_first, 96ull * t.items, l);
    wave_copy((const uint8_t*)t.midx, (uint8_t*)(d_midx + t.round_first), 4ull * t.items, l);
    wave_copy((const uint8_t*)t.cid, (uint8_t*)(d_cid + t.round_first), 4ull * t.items, l);
    const uint32_t dpi = bits_stride / 4;
    const int fast = stream_bits_fast(t.bits, t.bits_len);
    uint32_t* dst = (uint32_t*)(d_bits + (uint64_t)bits_stride * t.round_first);
    if ((uint64_t)t.items * dpi < 0xFFFFFF00ull) wave_restride<uint32_t>(t, dst, dpi, fast, l);
    else wave_restride<uint64_t>(t, dst, dpi, fast, l);
}

// One workgroup per tile of a device piece: result bytes and status words to caller + first, the accept bits into the caller's bitmap (words
// entirely inside the piece stored whole, boundary words OR-ed in: the call's other pieces own their other bits; the words were zeroed on the
// caller's stream at submit).
__global__ __launch_bounds__(SWG) void k_stream_scatter(const stile* __restrict__ tiles, const uint8_t* __restrict__ round_res, const uint32_t* __restrict__ round_st) {
    const stile t = tiles[blockIdx.x];
    const unsigned l = threadIdx.x;
    for (uint64_t i = l; i < t.items; i += SWG) {
        t.res[t.call_first + i] = round_res[t.round_first + i];
        if (t.st) t.st[t.call_first + i] = round_st[t.round_first + i];
    }
    if (t.bm) {
        uint64_t w0, nw; stream_bitmap_words(t.call_first, t.items, &w0, &nw);
        for (uint64_t j = l; j < nw; j += SWG) {
            int whole; const uint64_t bits = stream_bitmap_word(round_res, t.round_first, t.call_first, t.items, w0 + j, &whole);
            if (whole) t.bm[w0 + j] = bits;
            else if (bits) atomicOr((unsigned long long*)&t.bm[w0 + j], (unsigned long long)bits);
        }
    }
}

namespace {
// a tile of at most CMT_TILE sets of a verify_multiple call: the caller's five arrays at the tile's first set, and where its sets lie in the round
struct vtile { const uint8_t* sigs; const uint32_t* cid; const uint8_t* bits; const uint32_t* midx; const uint64_t* rands; uint32_t bits_len, items; uint64_t round_first; };
// a device call's outputs: sets [call_first, call_first + items) of the call are sets [round_first, ...) of the round; the tile at call_first = 0 also carries the
// call's batch byte and word, which the round keeps at n_round + batch
struct vstile { uint8_t* res; uint32_t* st; uint8_t* set_res; uint32_t* set_st; uint64_t call_first, items, round_first, batch_at; };
}  // namespace

// One workgroup per tile of a device call of a verify_multiple stream: signatures, set words, message indices and scalars copied to the round's arrays at
// round_first (wave_copy), the bitfields re-strided from bits_len bytes at any address to the slot's bits_stride (stream_bits_dword: every dword of every set's
// stride is written -- for bits_len = 0 zeros, and nothing is read --, so a slot never shows a round the bits or scalars of the round before).
__global__ __launch_bounds__(SWG) void k_stream_gather_vm(const vtile* __restrict__ tiles, uint8_t* __restrict__ d_sigs, uint32_t* __restrict__ d_cid,
                                                          uint8_t* __restrict__ d_bits, uint32_t* __restrict__ d_midx, uint64_t* __restrict__ d_rands, uint32_t bits_stride) {
    const vtile t = tiles[blockIdx.x];
    const unsigned l = threadIdx.x;
    wave_copy(t.sigs, d_sigs + 96 * t.round_first, 96ull * t.items, l);
    wave_copy((const uint8_t*)t.cid, (uint8_t*)(d_cid + t.round_first), 4ull * t.items, l);
    wave_copy((const uint8_t*)t.midx, (uint8_t*)(d_midx + t.round_first), 4ull * t.items, l);
    wave_copy((const uint8_t*)t.rands, (uint8_t*)(d_rands + t.round_first), 8ull * t.items, l);
    const uint32_t dpi = bits_stride / 4;
    const ctile c{t.sigs, t.midx, t.cid, t.bits, t.bits_len, t.items, t.round_first};
    const int fast = stream_bits_fast(t.bits, t.bits_len);
    uint32_t* dst = (uint32_t*)(d_bits + (uint64_t)bits_stride * t.round_first);
    if ((uint64_t)t.items * dpi < 0xFFFFFF00ull) wave_restride<uint32_t>(c, dst, dpi, fast, l);
    else wave_restride<uint64_t>(c, dst, dpi, fast, l);
}

// One workgroup per tile of a device call: the call's batch byte and word into the caller's output buffers (the first tile), its set bytes and words into the
// caller's arrays (either may be absent). round_res / round_st: the round's set outputs, with the batches' behind them.
__global__ __launch_bounds__(SWG) void k_stream_scatter_vm(const vstile* __restrict__ tiles, const uint8_t* __restrict__ round_res, const uint32_t* __restrict__ round_st) {
    const vstile t = tiles[blockIdx.x];
    const unsigned l = threadIdx.x;
    if (t.call_first == 0 && l == 0) {
        t.res[0] = round_res[t.batch_at];
        if (t.st) t.st[0] = round_st[t.batch_at];
    }
    if (!t.set_res && !t.set_st) return;
    for (uint64_t i = l; i < t.items; i += SWG) {
        if (t.set_res) t.set_res[t.call_first + i] = round_res[t.round_first + i];
        if (t.set_st) t.set_st[t.call_first + i] = round_st[t.round_first + i];
    }
}

namespace {

struct call_rec {
    uint64_t ticket = 0; bool host = false; bool split = false;
    mbls_stream_call_shape shape{};
    const uint8_t* sigs = nullptr; const uint8_t* msgs = nullptr; const uint8_t* keys = nullptr;   // keys: bytes or indices (a committee call: its committee ids)
    const uint8_t* bits = nullptr; uint32_t bits_len = 0;                     // a committee call: its bitfields, bits_len bytes per item
    uint8_t* res = nullptr; uint64_t* bm = nullptr; uint32_t* st = nullptr;
    hipEvent_t ev = nullptr;                                                 // device submits: recorded on the caller's stream
    // a verify_multiple call (shape.n sets; keys: its set words; res / st: ONE byte and word): its scalars, its per-set outputs, the groups it may form
    const uint64_t* rands = nullptr; uint8_t* set_res = nullptr; uint32_t* set_st = nullptr; uint64_t groups = 0;
};
struct piece_rec { std::shared_ptr<call_rec> c; uint64_t first, items, round_first; uint64_t batch = 0; };   // batch: a verify_multiple call's batch of the round

struct slot {
    uint8_t *d_sigs = nullptr, *d_msgs = nullptr, *d_keys = nullptr, *d_res = nullptr, *d_meta = nullptr; uint32_t* d_st = nullptr;
    uint8_t *h_meta = nullptr, *h_res = nullptr; uint32_t* h_st = nullptr;      // pinned
    uint32_t* d_cid = nullptr; uint8_t* h_bits = nullptr;                       // a committee stream: the round's committee ids (its fields lie in d_keys); pinned: host pieces' fields, zero-extended
    uint64_t* d_rands = nullptr; mbls_stream_vm_fill vfill{};                   // a verify_multiple stream: the round's scalars; its fill (fill.items mirrors vfill.cost)
    uint8_t* h_sigs = nullptr; uint64_t* h_rands = nullptr; uint32_t *h_cid = nullptr, *h_midx = nullptr;   // and the pinned mirrors of its host calls' arrays (one block: h_sigs)
    hipEvent_t gev = nullptr, done = nullptr;
    std::vector<piece_rec> pieces;
    mbls_stream_fill fill{};
    bool full = false;
    uint64_t first_ticket = 0, done_through = 0;
    int rc = MBLS_OK;
};

}  // namespace

struct mbls_stream {
    mbls_ctx* ctx = nullptr; const mbls_keytable* tab = nullptr;
    mbls_msgtable* mt = nullptr;                     // non-null: a message-table stream -- a call's "message bytes" are its uint32 table indices (msg_len = 4)
    mbls_committees* cm = nullptr; uint32_t bits_stride = 0; bool cm_bound = false;   // cm non-null: a committee stream (mt is set too) -- a call's keys are committee ids and bitfields
    bool vm = false;                                 // a verify_multiple stream (cm and mt are set): a call is a batch, a round one call of the batches entry
    int mode = 0, fmt = MBLS_PK_UNCOMPRESSED, dev = 0; size_t unit = 96;
    mbls_stream_opts o{};
    uint64_t meta_bytes = 0;
    hipStream_t hs = nullptr, gs = nullptr;
    std::vector<slot> slots;

    std::mutex mu;
    std::condition_variable cv_launch, cv_complete, cv_done;
    std::deque<std::shared_ptr<call_rec>> calls;     // submitted, not yet complete; calls[t - base] holds ticket t
    uint64_t base = 1, last_ticket = 0, cursor = 1, item_off = 0, flush_upto = 0, completed_through = 0, cut_done_through = 0;
    std::deque<int> free_slots, inflight;
    int open = -1;
    bool stop = false, closing = false, dead = false;
    int err_code = MBLS_OK; uint64_t err_ticket = 0;
    mbls_stream_stats stats{};
    std::vector<hipEvent_t> ev_pool;
    std::thread launcher, completer;
    std::mutex err_mu; char err[256] = "";
};

namespace {

int fail(mbls_stream* s, int rc, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int fail(mbls_stream* s, int rc, const char* fmt, ...) {
    std::lock_guard<std::mutex> g(s->err_mu);
    va_list ap; va_start(ap, fmt); vsnprintf(s->err, sizeof(s->err), fmt, ap); va_end(ap);
    return rc;
}

uint64_t meta_capacity(const mbls_stream_opts& o, size_t unit, bool committee, bool vm) {
    const uint64_t R = o.round_items;
    // a verify_multiple round: at most R / 2 calls; a call takes at most sets / tile + 1 gather tiles and as many scatter tiles; the batch table
    if (vm) return (R + R / CMT_TILE + 1) * sizeof(vtile) + (R + R / SCATTER_TILE + 1) * sizeof(vstile) + 4 * (R + 2) + 64;
    const uint64_t bytes = 96 * R + o.round_msg_bytes + unit * o.round_keys;
    const uint64_t ng = bytes / GATHER_TILE + 3 * R + 3, ns = 2 * R + R / SCATTER_TILE + 1;      // (a piece takes at most items / tile + 2 scatter tiles)
    const uint64_t nc = committee ? R + R / CMT_TILE + 1 : 0;                                    // (and at most items / tile + 1 committee tiles)
    return ng * sizeof(gtile) + ns * sizeof(stile) + nc * sizeof(ctile) + 4 * (R + 1) + 8 * (R + 1) + 64;
}

// The round in the open slot: gather, the device entry, scatter, completion event. Runs on the launcher thread without the stream's lock.
int launch_round(mbls_stream* s, slot& sl) {
    const uint64_t n = sl.fill.items;
    mbls_stream_layout lay{};
    for (size_t p = 0; p < sl.pieces.size(); p++) stream_layout_add(lay, p == 0, sl.pieces[p].c->shape);
    if (s->mode == MBLS_STREAM_VERIFY) { lay.keys_uniform = 1; lay.k = 1; }
    // the meta area, packed: gather tiles | scatter tiles | key offsets | message offsets -- one upload from pinned memory
    std::vector<gtile> gt; std::vector<stile> stv;
    std::vector<uint32_t> pkoff; std::vector<uint64_t> moff;
    if (!lay.keys_uniform) pkoff.resize(n + 1);
    if (!lay.msgs_uniform) moff.resize(n + 1);
    uint64_t key_cur = 0, msg_cur = 0, gathered = 0;
    bool any_host = false;
    hipError_t e = hipSuccess;
    auto seg = [&](bool host, const uint8_t* src, uint8_t* dst, uint64_t bytes) {
        if (!bytes) return;
        gathered += bytes;
        if (host) { if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s->gs); return; }
        for (uint64_t o = 0; o < bytes; o += GATHER_TILE) gt.push_back(gtile{src + o, dst + o, std::min(GATHER_TILE, bytes - o)});
    };
    hipEvent_t last_ev = nullptr;
    std::vector<ctile> ct;
    const uint64_t bs = s->bits_stride;
    for (const piece_rec& p : sl.pieces) {
        const call_rec& c = *p.c; const mbls_stream_call_shape& sh = c.shape;
        if (!c.host && c.ev != last_ev) { if (e == hipSuccess) e = hipStreamWaitEvent(s->gs, c.ev, 0); last_ev = c.ev; }
        any_host |= c.host;
        if (s->cm && !c.host) {       // a device piece of a committee call: one record per CMT_TILE items, the four arrays in one kernel (k_stream_gather_cmt)
            const uint32_t* midx = (const uint32_t*)c.msgs; const uint32_t* cid = (const uint32_t*)c.keys;
            for (uint64_t a = p.first; a < p.first + p.items; a += CMT_TILE)
                ct.push_back(ctile{c.sigs + 96 * a, midx + a, cid + a, c.bits + (uint64_t)c.bits_len * a, c.bits_len,
                                   (uint32_t)std::min(CMT_TILE, p.first + p.items - a), p.round_first + (a - p.first)});
            gathered += (96 + 4 + 4 + (uint64_t)c.bits_len) * p.items;
        } else if (s->cm) {           // a host piece: three plain copies, and the fields zero-extended to the stride on their way through pinned memory
            seg(true, c.sigs + 96 * p.first, sl.d_sigs + 96 * p.round_first, 96 * p.items);
            seg(true, c.msgs + 4 * p.first, sl.d_msgs + 4 * p.round_first, 4 * p.items);
            seg(true, c.keys + 4 * p.first, (uint8_t*)(sl.d_cid + p.round_first), 4 * p.items);
            uint8_t* hb = sl.h_bits + bs * p.round_first; const uint8_t* src = c.bits + (uint64_t)c.bits_len * p.first;
            if (c.bits_len == bs) memcpy(hb, src, bs * p.items);
            else for (uint64_t i = 0; i < p.items; i++) { memcpy(hb + bs * i, src + (uint64_t)c.bits_len * i, c.bits_len); memset(hb + bs * i + c.bits_len, 0, bs - c.bits_len); }
            seg(true, hb, sl.d_keys + bs * p.round_first, bs * p.items);
            gathered -= (bs - c.bits_len) * p.items;                // (the statistic counts the bytes the call carries)
        }
        if (!s->cm) {
        seg(c.host, c.sigs + 96 * p.first, sl.d_sigs + 96 * p.round_first, 96 * p.items);
        const uint64_t m0 = sh.msg_offsets ? sh.msg_offsets[p.first] : (uint64_t)sh.msg_len * p.first;
        const uint64_t mb = sh.msg_offsets ? sh.msg_offsets[p.first + p.items] - m0 : (uint64_t)sh.msg_len * p.items;
        seg(c.host, c.msgs + m0, sl.d_msgs + msg_cur, mb);
        const uint64_t k0 = sh.pk_offsets ? sh.pk_offsets[p.first] : (uint64_t)sh.k * p.first;
        const uint64_t kc = sh.pk_offsets ? sh.pk_offsets[p.first + p.items] - k0 : (uint64_t)sh.k * p.items;
        seg(c.host, c.keys + s->unit * k0, sl.d_keys + s->unit * key_cur, s->unit * kc);
        if (!lay.keys_uniform || !lay.msgs_uniform)
        for (uint64_t i = 0; i < p.items; i++) {
            if (!lay.keys_uniform) pkoff[p.round_first + i] = (uint32_t)(key_cur + (sh.pk_offsets ? sh.pk_offsets[p.first + i] - k0 : (uint64_t)sh.k * i));
            if (!lay.msgs_uniform) moff[p.round_first + i] = msg_cur + (sh.msg_offsets ? sh.msg_offsets[p.first + i] - m0 : (uint64_t)sh.msg_len * i);
        }
        key_cur += kc; msg_cur += mb;
        }
        if (!c.host)
            for (uint64_t a = p.first; a < p.first + p.items;) {
                const uint64_t b = std::min(p.first + p.items, (a / SCATTER_TILE + 1) * SCATTER_TILE);
                stv.push_back(stile{c.res, c.st, c.bm, a, b - a, p.round_first + (a - p.first)});
                a = b;
            }
    }
    if (!lay.keys_uniform) pkoff[n] = (uint32_t)key_cur;
    if (!lay.msgs_uniform) moff[n] = msg_cur;
    auto up = [](uint64_t x, uint64_t a) { return (x + a - 1) / a * a; };
    const uint64_t at_g = 0, at_s = up(at_g + gt.size() * sizeof(gtile), 16), at_k = up(at_s + stv.size() * sizeof(stile), 8), at_m = up(at_k + pkoff.size() * 4, 8);
    const uint64_t at_c = up(at_m + moff.size() * 8, 16), off = at_c + ct.size() * sizeof(ctile);
    if (off > s->meta_bytes) return fail(s, MBLS_ERR_DEVICE, "internal: round meta of %llu bytes exceeds the slot's %llu", (unsigned long long)off, (unsigned long long)s->meta_bytes);
    if (!gt.empty()) memcpy(sl.h_meta + at_g, gt.data(), gt.size() * sizeof(gtile));
    if (!stv.empty()) memcpy(sl.h_meta + at_s, stv.data(), stv.size() * sizeof(stile));
    if (!pkoff.empty()) memcpy(sl.h_meta + at_k, pkoff.data(), pkoff.size() * 4);
    if (!moff.empty()) memcpy(sl.h_meta + at_m, moff.data(), moff.size() * 8);
    if (!ct.empty()) memcpy(sl.h_meta + at_c, ct.data(), ct.size() * sizeof(ctile));
    if (e == hipSuccess && off) e = hipMemcpyAsync(sl.d_meta, sl.h_meta, off, hipMemcpyHostToDevice, s->gs);
    if (e == hipSuccess && !gt.empty()) { hipLaunchKernelGGL(k_stream_gather, dim3((unsigned)gt.size()), dim3(SWG), 0, s->gs, (const gtile*)(sl.d_meta + at_g)); e = hipGetLastError(); }
    if (e == hipSuccess && !ct.empty()) {
        hipLaunchKernelGGL(k_stream_gather_cmt, dim3((unsigned)ct.size()), dim3(SWG), 0, s->gs, (const ctile*)(sl.d_meta + at_c), sl.d_sigs, (uint32_t*)sl.d_msgs, sl.d_cid, sl.d_keys,
                           s->bits_stride);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(sl.gev, s->gs);
    if (e == hipSuccess) e = hipStreamWaitEvent(s->hs, sl.gev, 0);
    if (e != hipSuccess) return fail(s, MBLS_ERR_DEVICE, "gather: %s", hipGetErrorString(e));
    const uint64_t* d_moff = lay.msgs_uniform ? nullptr : (const uint64_t*)(sl.d_meta + at_m);
    const uint32_t* d_pkoff = lay.keys_uniform ? nullptr : (const uint32_t*)(sl.d_meta + at_k);
    const uint32_t msg_len = lay.msgs_uniform ? lay.msg_len : 0, k = lay.keys_uniform ? lay.k : 0;
    int rc;
    if (s->cm)           // the round's four arrays, dense in round order, every field at the stream's stride
        rc = mbls_fast_aggregate_verify_batch_committee_msgtable_device(s->ctx, s->cm, sl.d_sigs, s->mt, (const uint32_t*)sl.d_msgs, sl.d_cid, sl.d_keys, s->bits_stride, n,
                                                                        sl.d_res, nullptr, sl.d_st, s->hs);
    else if (s->mt) {    // the staged "message bytes" are the items' table indices, dense in round order (every call has msg_len = 4 and no offsets)
        const uint32_t* d_midx = (const uint32_t*)sl.d_msgs;
        if (s->mode == MBLS_STREAM_VERIFY)
            rc = mbls_verify_batch_msgtable_device(s->ctx, sl.d_sigs, s->mt, d_midx, sl.d_keys, s->fmt, n, sl.d_res, nullptr, sl.d_st, s->hs);
        else if (s->tab)
            rc = mbls_fast_aggregate_verify_batch_indexed_msgtable_device(s->ctx, s->tab, sl.d_sigs, s->mt, d_midx, (const uint32_t*)sl.d_keys, d_pkoff, n, k,
                                                                          sl.d_res, nullptr, sl.d_st, s->hs);
        else
            rc = mbls_fast_aggregate_verify_batch_msgtable_device(s->ctx, sl.d_sigs, s->mt, d_midx, sl.d_keys, s->fmt, d_pkoff, n, k, sl.d_res, nullptr, sl.d_st, s->hs);
    } else if (s->mode == MBLS_STREAM_VERIFY)
        rc = mbls_verify_batch_device(s->ctx, sl.d_sigs, sl.d_msgs, msg_len, d_moff, sl.d_keys, s->fmt, n, sl.d_res, nullptr, sl.d_st, s->hs);
    else if (s->tab)
        rc = mbls_fast_aggregate_verify_batch_indexed_device(s->ctx, s->tab, sl.d_sigs, sl.d_msgs, msg_len, d_moff, (const uint32_t*)sl.d_keys, d_pkoff, n, k,
                                                             sl.d_res, nullptr, sl.d_st, s->hs);
    else
        rc = mbls_fast_aggregate_verify_batch_device(s->ctx, sl.d_sigs, sl.d_msgs, msg_len, d_moff, sl.d_keys, s->fmt, d_pkoff, n, k, sl.d_res, nullptr, sl.d_st, s->hs);
    if (rc) return fail(s, rc, "round of %llu items: %s", (unsigned long long)n, mbls_last_error(s->ctx));
    if (!stv.empty()) { hipLaunchKernelGGL(k_stream_scatter, dim3((unsigned)stv.size()), dim3(SWG), 0, s->hs, (const stile*)(sl.d_meta + at_s), (const uint8_t*)sl.d_res, (const uint32_t*)sl.d_st); e = hipGetLastError(); }
    if (e == hipSuccess && any_host) e = hipMemcpyAsync(sl.h_res, sl.d_res, n, hipMemcpyDeviceToHost, s->hs);
    if (e == hipSuccess && any_host) e = hipMemcpyAsync(sl.h_st, sl.d_st, 4 * n, hipMemcpyDeviceToHost, s->hs);
    if (e == hipSuccess) e = hipEventRecord(sl.done, s->hs);
    if (e != hipSuccess) return fail(s, MBLS_ERR_DEVICE, "scatter: %s", hipGetErrorString(e));
    std::lock_guard<std::mutex> g(s->mu);
    s->stats.gathered_bytes += gathered;
    return MBLS_OK;
}

// The round of a verify_multiple stream: every piece is a whole call and a batch of the round. Gather (k_stream_gather_vm; host calls by copies, their fields
// zero-extended in pinned memory), the ragged batch table with the meta area, ONE call of the public batches entry over the slot, scatter (k_stream_scatter_vm;
// host calls through the pinned result areas). The slot keeps the sets' bytes and words at [0, n) of d_res / d_st and the batches' behind them at [n, n + B).
int launch_round_vm(mbls_stream* s, slot& sl) {
    const uint64_t n = sl.vfill.sets, B = sl.vfill.calls, bs = s->bits_stride;
    std::vector<vtile> vt; std::vector<vstile> stv;
    std::vector<uint64_t> sets(B); std::vector<uint32_t> boff(B + 1);
    uint64_t gathered = 0, max_groups = 0;
    bool any_host = false;
    hipError_t e = hipSuccess;
    hipEvent_t last_ev = nullptr;
    auto up_h = [&](const void* src, void* dst, uint64_t bytes) { if (bytes && e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s->gs); };
    // host calls: their five arrays are laid into the slot's pinned mirrors at their sets' places in the round (the fields zero-extended on the way), and every
    // RUN of neighbouring host calls goes up in five copies -- a round of small host calls would otherwise pay five pageable copies per call
    uint64_t run_lo = 0, run_hi = 0;
    auto flush_run = [&]() {
        const uint64_t a = run_lo, m = run_hi - run_lo;
        if (!m) return;
        up_h(sl.h_sigs + 96 * a, sl.d_sigs + 96 * a, 96 * m); up_h(sl.h_cid + a, sl.d_cid + a, 4 * m); up_h(sl.h_midx + a, sl.d_msgs + 4 * a, 4 * m);
        up_h(sl.h_rands + a, sl.d_rands + a, 8 * m); up_h(sl.h_bits + bs * a, sl.d_keys + bs * a, bs * m);
        run_lo = run_hi = 0;
    };
    for (const piece_rec& p : sl.pieces) {
        const call_rec& c = *p.c; const uint64_t m = p.items, r0 = p.round_first;
        sets[p.batch] = m; max_groups += c.groups;
        gathered += (96 + 4 + 4 + 8 + (uint64_t)c.bits_len) * m;
        if (c.host) {
            any_host = true;
            if (run_hi != r0) { flush_run(); run_lo = r0; }
            run_hi = r0 + m;
            memcpy(sl.h_sigs + 96 * r0, c.sigs, 96 * m); memcpy(sl.h_cid + r0, c.keys, 4 * m); memcpy(sl.h_midx + r0, c.msgs, 4 * m); memcpy(sl.h_rands + r0, c.rands, 8 * m);
            uint8_t* hb = sl.h_bits + bs * r0;
            if (c.bits_len == bs) { if (bs) memcpy(hb, c.bits, bs * m); }
            else for (uint64_t i = 0; i < m; i++) { if (c.bits_len) memcpy(hb + bs * i, c.bits + (uint64_t)c.bits_len * i, c.bits_len); memset(hb + bs * i + c.bits_len, 0, bs - c.bits_len); }
            continue;
        }
        flush_run();
        if (c.ev != last_ev) { if (e == hipSuccess) e = hipStreamWaitEvent(s->gs, c.ev, 0); last_ev = c.ev; }
        const uint32_t* cid = (const uint32_t*)c.keys; const uint32_t* midx = (const uint32_t*)c.msgs;
        for (uint64_t a = 0; a < m; a += CMT_TILE)
            vt.push_back(vtile{c.sigs + 96 * a, cid + a, c.bits_len ? c.bits + (uint64_t)c.bits_len * a : nullptr, midx + a, c.rands + a, c.bits_len,
                               (uint32_t)std::min(CMT_TILE, m - a), r0 + a});
        for (uint64_t a = 0; a < m; a += SCATTER_TILE)
            stv.push_back(vstile{c.res, c.st, c.set_res, c.set_st, a, std::min(SCATTER_TILE, m - a), r0 + a, n + p.batch});
    }
    flush_run();
    stream_vm_offsets(sets.data(), B, boff.data());
    auto up = [](uint64_t x, uint64_t a) { return (x + a - 1) / a * a; };
    const uint64_t at_v = 0, at_s = up(at_v + vt.size() * sizeof(vtile), 16), at_o = up(at_s + stv.size() * sizeof(vstile), 16), off = at_o + 4 * (B + 1);
    if (off > s->meta_bytes) return fail(s, MBLS_ERR_DEVICE, "internal: round meta of %llu bytes exceeds the slot's %llu", (unsigned long long)off, (unsigned long long)s->meta_bytes);
    if (!vt.empty()) memcpy(sl.h_meta + at_v, vt.data(), vt.size() * sizeof(vtile));
    if (!stv.empty()) memcpy(sl.h_meta + at_s, stv.data(), stv.size() * sizeof(vstile));
    memcpy(sl.h_meta + at_o, boff.data(), 4 * (B + 1));
    if (e == hipSuccess) e = hipMemcpyAsync(sl.d_meta, sl.h_meta, off, hipMemcpyHostToDevice, s->gs);
    if (e == hipSuccess && !vt.empty()) {
        hipLaunchKernelGGL(k_stream_gather_vm, dim3((unsigned)vt.size()), dim3(SWG), 0, s->gs, (const vtile*)(sl.d_meta + at_v), sl.d_sigs, sl.d_cid, sl.d_keys, (uint32_t*)sl.d_msgs,
                           sl.d_rands, s->bits_stride);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(sl.gev, s->gs);
    if (e == hipSuccess) e = hipStreamWaitEvent(s->hs, sl.gev, 0);
    if (e != hipSuccess) return fail(s, MBLS_ERR_DEVICE, "gather: %s", hipGetErrorString(e));
    const int rc = mbls_verify_multiple_batches_committee_msgtable_locate_device(s->ctx, s->cm, sl.d_sigs, sl.d_cid, sl.d_keys, s->bits_stride, s->mt, (const uint32_t*)sl.d_msgs,
                                                                                 sl.d_rands, n, (const uint32_t*)(sl.d_meta + at_o), 0, B, max_groups, sl.d_res + n, sl.d_st + n,
                                                                                 sl.d_res, sl.d_st, s->hs);
    if (rc) return fail(s, rc, "round of %llu sets in %llu batches: %s", (unsigned long long)n, (unsigned long long)B, mbls_last_error(s->ctx));
    if (!stv.empty()) { hipLaunchKernelGGL(k_stream_scatter_vm, dim3((unsigned)stv.size()), dim3(SWG), 0, s->hs, (const vstile*)(sl.d_meta + at_s), (const uint8_t*)sl.d_res, (const uint32_t*)sl.d_st); e = hipGetLastError(); }
    if (e == hipSuccess && any_host) e = hipMemcpyAsync(sl.h_res, sl.d_res, n + B, hipMemcpyDeviceToHost, s->hs);
    if (e == hipSuccess && any_host) e = hipMemcpyAsync(sl.h_st, sl.d_st, 4 * (n + B), hipMemcpyDeviceToHost, s->hs);
    if (e == hipSuccess) e = hipEventRecord(sl.done, s->hs);
    if (e != hipSuccess) return fail(s, MBLS_ERR_DEVICE, "scatter: %s", hipGetErrorString(e));
    std::lock_guard<std::mutex> g(s->mu);
    s->stats.gathered_bytes += gathered;
    return MBLS_OK;
}

// the same for a verify_multiple stream: whole calls only (stream_take_whole, the rule mbls_stream_cut_vm states as data); a call that does not fit closes the round
void absorb_vm(mbls_stream* s, slot& sl) {
    while (s->cursor <= s->last_ticket && !sl.full) {
        const std::shared_ptr<call_rec>& c = s->calls[s->cursor - s->base];
        if (sl.vfill.calls && sl.first_ticket <= s->flush_upto && c->ticket > s->flush_upto) break;
        const uint64_t before = sl.vfill.sets;
        if (!stream_take_whole(s->o, sl.vfill, c->shape.n)) { sl.full = true; break; }
        if (sl.pieces.empty()) sl.first_ticket = c->ticket;
        sl.pieces.push_back(piece_rec{c, 0, c->shape.n, before, sl.vfill.calls - 1});
        sl.fill.items = sl.vfill.cost;
        sl.done_through = c->ticket; s->cursor++;
        if (stream_vm_full(s->o, sl.vfill)) sl.full = true;
    }
}

// cut queued calls into the open slot (lock held): the same stream_take mbls_stream_cut runs, a flush boundary after call flush_upto
void absorb(mbls_stream* s, slot& sl) {
    if (s->vm) { absorb_vm(s, sl); return; }
    while (s->cursor <= s->last_ticket && !sl.full) {
        const std::shared_ptr<call_rec>& c = s->calls[s->cursor - s->base];
        if (sl.fill.items && sl.first_ticket <= s->flush_upto && c->ticket > s->flush_upto) break;
        const uint64_t before = sl.fill.items;
        const uint64_t t = stream_take(s->o, sl.fill, c->shape, s->item_off);
        if (t) {
            if (sl.pieces.empty()) sl.first_ticket = c->ticket;
            if (s->item_off) c->split = true;
            sl.pieces.push_back(piece_rec{c, s->item_off, t, before});
            s->item_off += t;
        }
        if (s->item_off == c->shape.n) { sl.done_through = c->ticket; s->cursor++; s->item_off = 0; }
        else sl.full = true;
        if (sl.fill.items == s->o.round_items) sl.full = true;
    }
}

void launcher_main(mbls_stream* s) {
    (void)hipSetDevice(s->dev);
    std::unique_lock<std::mutex> lk(s->mu);
    for (;;) {
        if (s->open < 0) {
            while (s->free_slots.empty() && !s->stop) s->cv_launch.wait(lk);
            if (s->stop) return;
            s->open = s->free_slots.front(); s->free_slots.pop_front();
            slot& o = s->slots[s->open];
            o.pieces.clear(); o.fill = mbls_stream_fill{}; o.vfill = mbls_stream_vm_fill{}; o.full = false; o.first_ticket = 0; o.done_through = s->cut_done_through; o.rc = MBLS_OK;
        }
        slot& o = s->slots[s->open];
        absorb(s, o);
        const bool flush = o.fill.items && o.first_ticket <= s->flush_upto;
        const bool wc = s->o.policy == MBLS_STREAM_WORK_CONSERVING && s->inflight.size() < s->o.depth;
        if (o.fill.items && (o.full || flush || wc)) {
            const int si = s->open; s->open = -1;
            s->cut_done_through = o.done_through;
            s->stats.rounds++; s->stats.full_rounds += o.full; s->stats.pieces += o.pieces.size();
            for (const piece_rec& p : o.pieces) if (p.first && p.c->split && p.first + p.items == p.c->shape.n) s->stats.split_calls++;
            const bool dead = s->dead;
            lk.unlock();
            int rc = dead ? MBLS_ERR_DEVICE : s->vm ? launch_round_vm(s, o) : launch_round(s, o);
            lk.lock();
            o.rc = rc;
            s->inflight.push_back(si);
            s->cv_complete.notify_one();
            continue;
        }
        if (s->stop) return;
        s->cv_launch.wait(lk);
    }
}

void completer_main(mbls_stream* s) {
    (void)hipSetDevice(s->dev);
    std::unique_lock<std::mutex> lk(s->mu);
    for (;;) {
        while (s->inflight.empty() && !s->stop) s->cv_complete.wait(lk);
        if (s->inflight.empty()) return;
        const int si = s->inflight.front();
        slot& sl = s->slots[si];
        lk.unlock();
        int rc = sl.rc;
        if (!rc) { const hipError_t e = hipEventSynchronize(sl.done); if (e != hipSuccess) rc = fail(s, MBLS_ERR_DEVICE, "round: %s", hipGetErrorString(e)); }
        if (!rc)
            for (const piece_rec& p : sl.pieces) {
                if (!p.c->host) continue;
                if (s->vm) {          // the call's batch byte and word (kept behind the round's sets), then its sets'
                    const uint64_t at = sl.vfill.sets + p.batch;
                    p.c->res[0] = sl.h_res[at];
                    if (p.c->st) p.c->st[0] = sl.h_st[at];
                    if (p.c->set_res) memcpy(p.c->set_res, sl.h_res + p.round_first, p.items);
                    if (p.c->set_st) memcpy(p.c->set_st, sl.h_st + p.round_first, 4 * p.items);
                    continue;
                }
                memcpy(p.c->res + p.first, sl.h_res + p.round_first, p.items);
                if (p.c->st) memcpy(p.c->st + p.first, sl.h_st + p.round_first, 4 * p.items);
            }
        lk.lock();
        if (rc) {
            s->dead = true;
            if (!s->err_code) { s->err_code = rc; s->err_ticket = sl.first_ticket; }
        }
        if (sl.done_through > s->completed_through) s->completed_through = sl.done_through;
        sl.pieces.clear();
        while (!s->calls.empty() && s->calls.front()->ticket <= s->completed_through && s->calls.front()->ticket < s->cursor) {
            if (s->calls.front()->ev) s->ev_pool.push_back(s->calls.front()->ev);
            if (s->mt) mblsi_msgtable_stream_calls(s->mt, -1);
            if (s->cm) mblsi_committees_stream_calls(s->cm, -1);
            s->calls.pop_front(); s->base++;
        }
        s->inflight.pop_front(); s->free_slots.push_back(si);
        s->cv_launch.notify_one(); s->cv_done.notify_all();
    }
}

void free_stream(mbls_stream* s) {
    for (slot& sl : s->slots) {
        for (uint8_t* p : {sl.d_sigs, sl.d_msgs, sl.d_keys, sl.d_res, sl.d_meta}) if (p) (void)hipFree(p);
        if (sl.d_st) (void)hipFree(sl.d_st);
        if (sl.d_cid) (void)hipFree(sl.d_cid);
        if (sl.d_rands) (void)hipFree(sl.d_rands);
        for (void* p : {(void*)sl.h_meta, (void*)sl.h_res, (void*)sl.h_st, (void*)sl.h_bits, (void*)sl.h_sigs}) if (p) (void)hipHostFree(p);
        if (sl.gev) (void)hipEventDestroy(sl.gev);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    for (hipEvent_t ev : s->ev_pool) (void)hipEventDestroy(ev);
    for (auto& c : s->calls) if (c->ev) (void)hipEventDestroy(c->ev);
    if (s->hs) (void)hipStreamDestroy(s->hs);
    if (s->gs) (void)hipStreamDestroy(s->gs);
    if (s->cm_bound) mblsi_committees_stream_unbind(s->cm, s->bits_stride);
    delete s;
}

// the call joins the queue: a device submit zeroes its bitmap words and records its event on the caller's stream first
int enqueue(mbls_stream* s, const std::shared_ptr<call_rec>& c, void* stream, uint64_t* ticket) {
    const uint64_t n = c->shape.n;
    if (!c->host) {
        {
            std::lock_guard<std::mutex> g(s->mu);
            if (!s->ev_pool.empty()) { c->ev = s->ev_pool.back(); s->ev_pool.pop_back(); }
        }
        hipError_t e = hipSetDevice(s->dev);
        if (e == hipSuccess && !c->ev) e = hipEventCreateWithFlags(&c->ev, hipEventDisableTiming);
        if (e == hipSuccess && c->bm) e = hipMemsetAsync(c->bm, 0, 8 * ((n + 63) / 64), (hipStream_t)stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev, (hipStream_t)stream);
        if (e != hipSuccess) {
            if (c->ev) { std::lock_guard<std::mutex> g(s->mu); s->ev_pool.push_back(c->ev); }
            return fail(s, MBLS_ERR_DEVICE, "submit: %s", hipGetErrorString(e));
        }
    }
    std::lock_guard<std::mutex> g(s->mu);
    if (s->dead || s->closing) {
        if (c->ev) s->ev_pool.push_back(c->ev);
        return s->dead ? fail(s, MBLS_ERR_DEVICE, "the stream met a device error") : fail(s, MBLS_ERR_ARGUMENT, "the stream is being destroyed");
    }
    c->ticket = ++s->last_ticket;
    s->calls.push_back(c);
    if (s->mt) mblsi_msgtable_stream_calls(s->mt, 1);
    if (s->cm) mblsi_committees_stream_calls(s->cm, 1);
    s->stats.calls++; s->stats.items += n;
    *ticket = c->ticket;
    s->cv_launch.notify_one();
    return MBLS_OK;
}

int submit(mbls_stream* s, bool msgidx, bool host, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff, const uint8_t* pks,
           const uint32_t* idx, const uint32_t* poff, uint64_t n, uint32_t k, uint8_t* res, uint64_t* bm, uint32_t* st, void* stream, uint64_t* ticket) {
    if (!s) return MBLS_ERR_ARGUMENT;
    if (!ticket) return fail(s, MBLS_ERR_ARGUMENT, "null ticket pointer");
    if (s->vm) return fail(s, MBLS_ERR_ARGUMENT, "a verify_multiple stream takes whole batches of sets (mbls_stream_submit_vm[_device])");
    if (s->cm) return fail(s, MBLS_ERR_ARGUMENT, "a committee stream takes committee ids and bitfields (mbls_stream_submit_committee[_device])");
    if (msgidx != (s->mt != nullptr))
        return fail(s, MBLS_ERR_ARGUMENT, s->mt ? "a message-table stream takes message indices (mbls_stream_submit_msgidx[_device])"
                                                : "this stream takes messages, not message-table indices (mbls_stream_submit[_device])");
    if (n == 0) return fail(s, MBLS_ERR_ARGUMENT, "a call holds at least one item");
    if (!sigs || !res) return fail(s, MBLS_ERR_ARGUMENT, "null buffer");
    if (s->mode == MBLS_STREAM_VERIFY && (poff || k != 1)) return fail(s, MBLS_ERR_ARGUMENT, "verify mode: one key per item (k = 1, no key offsets)");
    if (s->tab ? pks != nullptr : idx != nullptr)
        return fail(s, MBLS_ERR_ARGUMENT, s->tab ? "an index stream takes key indices, not key bytes" : "a byte-key stream takes key bytes, not key indices");
    mbls_stream_call_shape sh{n, k, msg_len, poff, moff, 0};
    int what = 0; const uint64_t bad = stream_check_call(s->o, sh, &what);
    if (bad) {
        const uint64_t i = bad - 1;
        if (what == 1) return fail(s, MBLS_ERR_ARGUMENT, "offset table runs backwards (or holds a message of 2^32 bytes or more) at item %llu", (unsigned long long)i);
        if (what == 2) return fail(s, MBLS_ERR_ARGUMENT, "item %llu has %llu keys; a round holds %llu (mbls_stream_opts.round_keys)", (unsigned long long)i,
                                   (unsigned long long)stream_item_keys(sh, i), (unsigned long long)s->o.round_keys);
        return fail(s, MBLS_ERR_ARGUMENT, "item %llu has a %llu-byte message; a round holds %llu message bytes (mbls_stream_opts.round_msg_bytes)", (unsigned long long)i,
                    (unsigned long long)stream_item_msg(sh, i), (unsigned long long)s->o.round_msg_bytes);
    }
    const uint64_t msg_total = moff ? moff[n] - moff[0] : (uint64_t)msg_len * n;
    const uint64_t key_total = poff ? (uint64_t)(poff[n] - poff[0]) : (uint64_t)k * n;
    if (msg_total && !msgs) return fail(s, MBLS_ERR_ARGUMENT, "null message buffer");
    if (key_total && !(s->tab ? (const void*)idx : (const void*)pks)) return fail(s, MBLS_ERR_ARGUMENT, "null key buffer");
    auto c = std::make_shared<call_rec>();
    c->host = host; c->shape = sh; c->sigs = sigs; c->msgs = msgs; c->keys = s->tab ? (const uint8_t*)idx : pks; c->res = res; c->bm = bm; c->st = st;
    return enqueue(s, c, stream, ticket);
}

// a committee call: the shape {n, k = 0, msg_len = 4} -- the message indices are its "message bytes", as on a message-table stream; ids and fields ride along
int submit_cmt(mbls_stream* s, bool host, const uint8_t* sigs, const uint32_t* msg_idx, const uint32_t* cmt_idx, const uint8_t* bits, uint32_t bits_len, uint64_t n,
               uint8_t* res, uint64_t* bm, uint32_t* st, void* stream, uint64_t* ticket) {
    if (!s) return MBLS_ERR_ARGUMENT;
    if (!ticket) return fail(s, MBLS_ERR_ARGUMENT, "null ticket pointer");
    if (s->vm) return fail(s, MBLS_ERR_ARGUMENT, "a verify_multiple stream takes whole batches of sets (mbls_stream_submit_vm[_device])");
    if (!s->cm)
        return fail(s, MBLS_ERR_ARGUMENT, s->mt ? "this is not a committee stream: a message-table stream takes mbls_stream_submit_msgidx[_device]"
                                                : "this is not a committee stream: it takes messages and keys (mbls_stream_submit[_device])");
    if (n == 0) return fail(s, MBLS_ERR_ARGUMENT, "a call holds at least one item");
    if (!sigs || !res || !msg_idx || !cmt_idx || !bits) return fail(s, MBLS_ERR_ARGUMENT, "null buffer");
    if (bits_len == 0 || bits_len > s->bits_stride)
        return fail(s, MBLS_ERR_ARGUMENT, "bits_len is %u; a field holds 1 to %u bytes (the stream's bits_stride)", bits_len, s->bits_stride);
    mbls_stream_call_shape sh{n, 0, 4, nullptr, nullptr, 0};
    int what = 0;
    if (stream_check_call(s->o, sh, &what))
        return fail(s, MBLS_ERR_ARGUMENT, "an item takes 4 message bytes; a round holds %llu (mbls_stream_opts.round_msg_bytes)", (unsigned long long)s->o.round_msg_bytes);
    auto c = std::make_shared<call_rec>();
    c->host = host; c->shape = sh; c->sigs = sigs; c->msgs = (const uint8_t*)msg_idx; c->keys = (const uint8_t*)cmt_idx; c->bits = bits; c->bits_len = bits_len;
    c->res = res; c->bm = bm; c->st = st;
    return enqueue(s, c, stream, ticket);
}

// a verify_multiple call: one batch of n sets, never split (shape.n = its sets; the cutting reads nothing else of the shape)
int submit_vm(mbls_stream* s, bool host, const uint8_t* sigs, const uint32_t* cmt_idx, const uint8_t* bits, uint32_t bits_len, const uint32_t* msg_idx, const uint64_t* rands,
              uint64_t n, uint8_t* res, uint32_t* st, uint8_t* set_res, uint32_t* set_st, void* stream, uint64_t* ticket) {
    if (!s) return MBLS_ERR_ARGUMENT;
    if (!ticket) return fail(s, MBLS_ERR_ARGUMENT, "null ticket pointer");
    if (!s->vm)
        return fail(s, MBLS_ERR_ARGUMENT, s->cm   ? "this is not a verify_multiple stream: a committee stream takes mbls_stream_submit_committee[_device]"
                                          : s->mt ? "this is not a verify_multiple stream: a message-table stream takes mbls_stream_submit_msgidx[_device]"
                                                  : "this is not a verify_multiple stream: it takes messages and keys (mbls_stream_submit[_device])");
    if (n == 0) return fail(s, MBLS_ERR_ARGUMENT, "a call holds at least one set");
    if (!rands) return fail(s, MBLS_ERR_ARGUMENT, "verify_multiple without blinding scalars is forgeable: rands must not be NULL");
    if (!sigs || !res || !msg_idx || !cmt_idx) return fail(s, MBLS_ERR_ARGUMENT, "null buffer");
    if (bits_len > s->bits_stride) return fail(s, MBLS_ERR_ARGUMENT, "bits_len is %u; a field holds 0 to %u bytes (the stream's bits_stride)", bits_len, s->bits_stride);
    if (bits_len && !bits) return fail(s, MBLS_ERR_ARGUMENT, "null bitfields with bits_len = %u (only bits_len = 0 allows it)", bits_len);
    if (!stream_vm_fits(s->o, n))
        return fail(s, MBLS_ERR_ARGUMENT, "a call of %llu sets costs %llu of a round; a round holds %llu (mbls_stream_opts.round_items): at most %llu sets per call",
                    (unsigned long long)n, (unsigned long long)stream_vm_cost(n), (unsigned long long)s->o.round_items, (unsigned long long)(s->o.round_items - 1));
    auto c = std::make_shared<call_rec>();
    c->host = host; c->shape = mbls_stream_call_shape{n, 0, 4, nullptr, nullptr, 0};
    c->sigs = sigs; c->msgs = (const uint8_t*)msg_idx; c->keys = (const uint8_t*)cmt_idx; c->bits = bits; c->bits_len = bits_len; c->rands = rands;
    c->res = res; c->st = st; c->set_res = set_res; c->set_st = set_st;
    // the groups the call may form in the round's group space: a host call's distinct message indices, counted as the batches entry counts them (a batch above the
    // grouping cap has one group per set); a device call's indices cannot be seen here
    c->groups = n;
    if (host && n <= MBLS_VBG_MAX_SETS) {
        std::vector<uint32_t> seen;
        try { seen.assign(msg_idx, msg_idx + n); } catch (...) { return fail(s, MBLS_ERR_DEVICE, "out of host memory"); }
        std::sort(seen.begin(), seen.end());
        c->groups = (uint64_t)(std::unique(seen.begin(), seen.end()) - seen.begin());
    }
    return enqueue(s, c, stream, ticket);
}

}  // namespace

extern "C" int mbls_stream_cut_vm(const mbls_stream_opts* o, const uint64_t* call_sets, const uint32_t* flush_after, uint64_t n_calls, mbls_stream_piece* out,
                                  uint64_t max_pieces, uint64_t* n_pieces) {
    if (!o || !call_sets || !n_calls || !n_pieces || !o->round_items || (!out && max_pieces)) return MBLS_ERR_ARGUMENT;
    for (uint64_t j = 0; j < n_calls; j++) if (!stream_vm_fits(*o, call_sets[j])) return MBLS_ERR_ARGUMENT;
    mbls_stream_vm_fill f{}; uint64_t round = 0;
    for (uint64_t j = 0; j < n_calls; j++) {
        uint64_t before = f.sets;
        if (!stream_take_whole(*o, f, call_sets[j])) {            // the call closes the open round and is the first of the next
            round++; f = mbls_stream_vm_fill{}; before = 0;
            (void)stream_take_whole(*o, f, call_sets[j]);
        }
        if (j < max_pieces) out[j] = mbls_stream_piece{j, 0, call_sets[j], round, before};
        if ((flush_after && flush_after[j]) || stream_vm_full(*o, f)) { round++; f = mbls_stream_vm_fill{}; }
    }
    *n_pieces = n_calls;
    return n_calls <= max_pieces || !out ? MBLS_OK : MBLS_ERR_ARGUMENT;
}

extern "C" int mbls_stream_cut(const mbls_stream_opts* o, const mbls_stream_call_shape* calls, uint64_t n_calls, mbls_stream_piece* out, uint64_t max_pieces,
                               uint64_t* n_pieces) {
    if (!o || !calls || !n_calls || !n_pieces || !o->round_items || !o->round_keys || !o->round_msg_bytes || (!out && max_pieces)) return MBLS_ERR_ARGUMENT;
    for (uint64_t j = 0; j < n_calls; j++) {
        int what; if (!calls[j].n || stream_check_call(*o, calls[j], &what)) return MBLS_ERR_ARGUMENT;
    }
    mbls_stream_fill f{}; uint64_t round = 0, np = 0;
    for (uint64_t j = 0; j < n_calls; j++) {
        uint64_t first = 0;
        while (first < calls[j].n) {
            const uint64_t before = f.items, t = stream_take(*o, f, calls[j], first);
            if (t) { if (np < max_pieces) out[np] = mbls_stream_piece{j, first, t, round, before}; np++; first += t; }
            if (first < calls[j].n || f.items == o->round_items) { round++; f = mbls_stream_fill{}; }
        }
        if (calls[j].flush_after && f.items) { round++; f = mbls_stream_fill{}; }
    }
    *n_pieces = np;
    return np <= max_pieces || !out ? MBLS_OK : MBLS_ERR_ARGUMENT;
}

static int stream_create(mbls_ctx* ctx, int mode, int pk_format, const mbls_keytable* t, mbls_msgtable* mt, mbls_committees* cm, uint32_t bits_stride,
                         bool vm, const mbls_stream_opts* opts, mbls_stream** out) {
    if (!ctx || !out) return MBLS_ERR_ARGUMENT;
    *out = nullptr;
    if (mode != MBLS_STREAM_FAST_AGGREGATE_VERIFY && mode != MBLS_STREAM_VERIFY) return MBLS_ERR_ARGUMENT;
    if (t && mode != MBLS_STREAM_FAST_AGGREGATE_VERIFY) return MBLS_ERR_ARGUMENT;           // only fast_aggregate_verify has an indexed entry
    if (!t && pk_format != MBLS_PK_COMPRESSED && pk_format != MBLS_PK_UNCOMPRESSED) return MBLS_ERR_ARGUMENT;
    // a table of another context is refused by the indexed entry itself (an empty call enqueues nothing)
    if (t && mbls_fast_aggregate_verify_batch_indexed_device(ctx, t, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr))
        return MBLS_ERR_ARGUMENT;
    // likewise a message table of another context, by the table entry itself
    if (mt && mbls_verify_batch_msgtable_device(ctx, nullptr, mt, nullptr, nullptr, MBLS_PK_UNCOMPRESSED, 0, nullptr, nullptr, nullptr, nullptr)) return MBLS_ERR_ARGUMENT;
    mbls_limits L; int rc = mbls_ctx_get_limits(ctx, &L); if (rc) return rc;
    mbls_stream_opts o = opts ? *opts : mbls_stream_opts{};
    if (o.policy != MBLS_STREAM_WORK_CONSERVING && o.policy != MBLS_STREAM_FULL_ROUNDS) return MBLS_ERR_ARGUMENT;
    if (!o.round_items) o.round_items = L.round_items;
    if (!o.round_keys) o.round_keys = (mode == MBLS_STREAM_VERIFY ? 1 : 128) * o.round_items;
    if (!o.round_msg_bytes) o.round_msg_bytes = (mt ? 4 : 64) * o.round_items;
    if (!o.depth) o.depth = 2;
    if (o.round_items > (1ull << 31) || o.round_keys > 0xFFFFFFFFull || o.depth > 64) return MBLS_ERR_ARGUMENT;    // key offsets of a round are 32-bit
    if (vm && o.round_items < 2) return MBLS_ERR_ARGUMENT;                  // the smallest call, one set and its signature pair, costs 2
    mbls_stream* s = new (std::nothrow) mbls_stream();
    if (!s) return MBLS_ERR_DEVICE;
    s->ctx = ctx; s->tab = t; s->mt = mt; s->mode = mode; s->fmt = t ? MBLS_PK_UNCOMPRESSED : pk_format; s->o = o;
    s->vm = vm;
    s->unit = cm ? 0 : t ? 4 : (pk_format == MBLS_PK_COMPRESSED ? 48 : 96);
    if (cm) {            // the table against this context and stride, and from here on its appends against the stride (released by free_stream)
        rc = mblsi_committees_stream_bind(ctx, cm, bits_stride);
        if (rc) { delete s; return rc; }
        s->cm = cm; s->bits_stride = bits_stride; s->cm_bound = true;
    }
    // every round size's workspace up front (a partial round on the wave engine may take the eight-lane key sum, n + 8 n items): no round grows it
    uint64_t ws = 0;
    const uint32_t kmax = (uint32_t)std::min<uint64_t>(o.round_keys, 0xFFFFFFFFull);
    for (uint64_t n = 1; n <= o.round_items && !vm; n++) {
        ws = std::max(ws, mbls_plan_workspace_items(&L, n, kmax, 1));
        if (kmax >= 32) ws = std::max(ws, mbls_plan_workspace_items(&L, n, 32, 1));
        if (cm) ws = std::max(ws, mbls_plan_workspace_items(&L, n, 0, 0));
    }
    // a verify_multiple round holds B batches of n sets in all with n + B <= round_items and B <= n. What the batches entry reserves
    // (mbls_plan_verify_multiple_batches_committee) does not decrease in n, in B or in the bound on the groups, and the bound is at most n: so the largest of every
    // (n, B) a round can hold lies on n = round_items - B, with no promise on the groups and a table that caps nothing, on either route, with locate
    for (uint64_t B = 1; vm && 2 * B <= o.round_items; B++)
        for (int route = 1; route <= 2; route++) {
            mbls_vm_batches_committee_plan vp;
            if (!mbls_plan_verify_multiple_batches_committee(&L, o.round_items - B, B, 0, 0xFFFFFFFFull, 0, route, 1, &vp)) ws = std::max(ws, vp.workspace_items);
        }
    rc = mbls_ctx_reserve(ctx, ws);                       // (leaves the context's device current on this thread)
    if (!rc && !t && !cm && pk_format == MBLS_PK_COMPRESSED) rc = mbls_ctx_reserve_keys(ctx, o.round_keys);
    // the index lists k_cmt_expand writes for a full round of the largest committees the stride admits
    if (!rc && cm) rc = mbls_ctx_reserve_committee_items(ctx, o.round_items, (uint32_t)std::min<uint64_t>(8ull * bits_stride, MBLS_COMMITTEE_MAX_MEMBERS));
    // the batches entry's own grow-only staging: the set map of a ragged batch table and the group arrays, for the most sets and batches a round holds
    if (!rc && vm) rc = mblsi_vbg_reserve_staging(ctx, o.round_items - 1, o.round_items / 2);
    if (rc) { free_stream(s); return rc; }
    hipError_t e = hipGetDevice(&s->dev);
    s->meta_bytes = meta_capacity(o, s->unit, cm != nullptr, vm);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->hs, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->gs, hipStreamNonBlocking);
    s->slots.resize(o.depth + 1);
    for (slot& sl : s->slots) {
        if (e == hipSuccess) e = hipMalloc(&sl.d_sigs, 96 * o.round_items);
        if (e == hipSuccess) e = hipMalloc(&sl.d_msgs, std::max<uint64_t>(vm ? 4 * o.round_items : o.round_msg_bytes, 16));
        if (e == hipSuccess && vm) e = hipMalloc(&sl.d_rands, 8 * o.round_items);
        if (e == hipSuccess && vm) {      // signatures | scalars | set words | message indices, each at its alignment
            e = hipHostMalloc((void**)&sl.h_sigs, (96 + 8 + 4 + 4) * o.round_items, hipHostMallocDefault);
            if (e == hipSuccess) { sl.h_rands = (uint64_t*)(sl.h_sigs + 96 * o.round_items); sl.h_cid = (uint32_t*)(sl.h_rands + o.round_items); sl.h_midx = sl.h_cid + o.round_items; }
        }
        if (e == hipSuccess) e = hipMalloc(&sl.d_keys, std::max<uint64_t>(cm ? (uint64_t)bits_stride * o.round_items : s->unit * o.round_keys, 16));
        if (e == hipSuccess && cm) e = hipMalloc(&sl.d_cid, 4 * o.round_items);
        if (e == hipSuccess && cm) e = hipHostMalloc((void**)&sl.h_bits, std::max<uint64_t>((uint64_t)bits_stride * o.round_items, 16), hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc(&sl.d_res, o.round_items);
        if (e == hipSuccess) e = hipMalloc(&sl.d_st, 4 * o.round_items);
        if (e == hipSuccess) e = hipMalloc(&sl.d_meta, s->meta_bytes);
        if (e == hipSuccess) e = hipHostMalloc((void**)&sl.h_meta, s->meta_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void**)&sl.h_res, o.round_items, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void**)&sl.h_st, 4 * o.round_items, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.gev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming | hipEventBlockingSync);
    }
    if (e != hipSuccess) { free_stream(s); return MBLS_ERR_DEVICE; }
    for (int i = 0; i < (int)s->slots.size(); i++) s->free_slots.push_back(i);
    try {
        s->launcher = std::thread(launcher_main, s);
        s->completer = std::thread(completer_main, s);
    } catch (...) {
        { std::lock_guard<std::mutex> g(s->mu); s->stop = true; }
        s->cv_launch.notify_all(); s->cv_complete.notify_all();
        if (s->launcher.joinable()) s->launcher.join();
        free_stream(s); return MBLS_ERR_DEVICE;
    }
    *out = s;
    return MBLS_OK;
}

extern "C" int mbls_stream_create(mbls_ctx* ctx, int mode, int pk_format, const mbls_keytable* t, const mbls_stream_opts* opts, mbls_stream** out) {
    return stream_create(ctx, mode, pk_format, t, nullptr, nullptr, 0, false, opts, out);
}
extern "C" int mbls_stream_create_msgtable(mbls_ctx* ctx, int mode, int pk_format, const mbls_keytable* t, mbls_msgtable* mt, const mbls_stream_opts* opts, mbls_stream** out) {
    if (!mt) return MBLS_ERR_ARGUMENT;
    return stream_create(ctx, mode, pk_format, t, mt, nullptr, 0, false, opts, out);
}
// a committee stream: fast_aggregate_verify over the committee table (and through it its key table) and the message table
extern "C" int mbls_stream_create_committee(mbls_ctx* ctx, mbls_committees* committees, mbls_msgtable* mt, uint32_t bits_stride, const mbls_stream_opts* opts,
                                            mbls_stream** out) {
    if (!committees || !mt) return MBLS_ERR_ARGUMENT;
    return stream_create(ctx, MBLS_STREAM_FAST_AGGREGATE_VERIFY, MBLS_PK_UNCOMPRESSED, nullptr, mt, committees, bits_stride, false, opts, out);
}
// a verify_multiple stream over the same two tables: a call is a batch, a round one call of mbls_verify_multiple_batches_committee_msgtable_locate_device
extern "C" int mbls_stream_create_vm_committee(mbls_ctx* ctx, mbls_committees* committees, mbls_msgtable* mt, uint32_t bits_stride, const mbls_stream_opts* opts,
                                               mbls_stream** out) {
    if (!committees || !mt) return MBLS_ERR_ARGUMENT;
    return stream_create(ctx, MBLS_STREAM_FAST_AGGREGATE_VERIFY, MBLS_PK_UNCOMPRESSED, nullptr, mt, committees, bits_stride, true, opts, out);
}

extern "C" void mbls_stream_destroy(mbls_stream* s) {
    if (!s) return;
    {
        std::unique_lock<std::mutex> lk(s->mu);
        s->closing = true;
        s->flush_upto = s->last_ticket;
        s->cv_launch.notify_one();
        while (s->completed_through < s->last_ticket) s->cv_done.wait(lk);
        s->stop = true;
    }
    s->cv_launch.notify_all(); s->cv_complete.notify_all();
    s->launcher.join(); s->completer.join();
    (void)hipSetDevice(s->dev);
    (void)hipStreamSynchronize(s->gs); (void)hipStreamSynchronize(s->hs);
    free_stream(s);
}

extern "C" const char* mbls_stream_last_error(mbls_stream* s) { return s ? s->err : "null stream"; }

extern "C" int mbls_stream_submit_device(mbls_stream* s, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* h_msg_offsets,
                                         const uint8_t* d_pks, const uint32_t* d_key_idx, const uint32_t* h_pk_offsets, uint64_t n, uint32_t k,
                                         uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream, uint64_t* ticket) {
    return submit(s, false, false, d_sigs, d_msgs, msg_len, h_msg_offsets, d_pks, d_key_idx, h_pk_offsets, n, k, d_results, d_bitmap, d_status, stream, ticket);
}

extern "C" int mbls_stream_submit(mbls_stream* s, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* msg_offsets,
                                  const uint8_t* pks, const uint32_t* key_idx, const uint32_t* pk_offsets, uint64_t n, uint32_t k,
                                  uint8_t* results, uint32_t* status, uint64_t* ticket) {
    return submit(s, false, true, sigs, msgs, msg_len, msg_offsets, pks, key_idx, pk_offsets, n, k, results, nullptr, status, nullptr, ticket);
}

// message-table streams: the index array travels as the call's message bytes, 4 per item
extern "C" int mbls_stream_submit_msgidx_device(mbls_stream* s, const uint8_t* d_sigs, const uint32_t* d_msg_idx, const uint8_t* d_pks, const uint32_t* d_key_idx,
                                                const uint32_t* h_pk_offsets, uint64_t n, uint32_t k, uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status,
                                                void* stream, uint64_t* ticket) {
    return submit(s, true, false, d_sigs, (const uint8_t*)d_msg_idx, 4, nullptr, d_pks, d_key_idx, h_pk_offsets, n, k, d_results, d_bitmap, d_status, stream, ticket);
}
extern "C" int mbls_stream_submit_msgidx(mbls_stream* s, const uint8_t* sigs, const uint32_t* msg_idx, const uint8_t* pks, const uint32_t* key_idx,
                                         const uint32_t* pk_offsets, uint64_t n, uint32_t k, uint8_t* results, uint32_t* status, uint64_t* ticket) {
    return submit(s, true, true, sigs, (const uint8_t*)msg_idx, 4, nullptr, pks, key_idx, pk_offsets, n, k, results, nullptr, status, nullptr, ticket);
}

// committee streams: the index array travels as the call's message bytes, the ids and fields beside it
extern "C" int mbls_stream_submit_committee_device(mbls_stream* s, const uint8_t* d_sigs, const uint32_t* d_msg_idx, const uint32_t* d_cmt_idx, const uint8_t* d_bits,
                                                   uint32_t bits_len, uint64_t n, uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream, uint64_t* ticket) {
    return submit_cmt(s, false, d_sigs, d_msg_idx, d_cmt_idx, d_bits, bits_len, n, d_results, d_bitmap, d_status, stream, ticket);
}
extern "C" int mbls_stream_submit_committee(mbls_stream* s, const uint8_t* sigs, const uint32_t* msg_idx, const uint32_t* cmt_idx, const uint8_t* bits, uint32_t bits_len,
                                            uint64_t n, uint8_t* results, uint32_t* status, uint64_t* ticket) {
    return submit_cmt(s, true, sigs, msg_idx, cmt_idx, bits, bits_len, n, results, nullptr, status, nullptr, ticket);
}

// verify_multiple streams: a call is one batch of n_sets sets; one byte and word per call, n_sets bytes and words per set
extern "C" int mbls_stream_submit_vm_device(mbls_stream* s, const uint8_t* d_sigs96, const uint32_t* d_cmt_idx, const uint8_t* d_bits, uint32_t bits_len,
                                            const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n_sets, uint8_t* d_result, uint32_t* d_status,
                                            uint8_t* d_set_results, uint32_t* d_set_status, void* stream, uint64_t* ticket) {
    return submit_vm(s, false, d_sigs96, d_cmt_idx, d_bits, bits_len, d_msg_idx, d_rands, n_sets, d_result, d_status, d_set_results, d_set_status, stream, ticket);
}
extern "C" int mbls_stream_submit_vm(mbls_stream* s, const uint8_t* sigs96, const uint32_t* cmt_idx, const uint8_t* bits, uint32_t bits_len, const uint32_t* msg_idx,
                                     const uint64_t* rands, uint64_t n_sets, uint8_t* result, uint32_t* status, uint8_t* set_results, uint32_t* set_status,
                                     uint64_t* ticket) {
    return submit_vm(s, true, sigs96, cmt_idx, bits, bits_len, msg_idx, rands, n_sets, result, status, set_results, set_status, nullptr, ticket);
}

extern "C" int mbls_stream_flush(mbls_stream* s) {
    if (!s) return MBLS_ERR_ARGUMENT;
    std::lock_guard<std::mutex> g(s->mu);
    s->flush_upto = s->last_ticket;
    s->cv_launch.notify_one();
    return MBLS_OK;
}

extern "C" int mbls_stream_wait(mbls_stream* s, uint64_t ticket) {
    if (!s) return MBLS_ERR_ARGUMENT;
    std::unique_lock<std::mutex> lk(s->mu);
    if (!ticket || ticket > s->last_ticket) return fail(s, MBLS_ERR_ARGUMENT, "unknown ticket %llu", (unsigned long long)ticket);
    if (s->completed_through < ticket) {
        if (s->flush_upto < ticket) { s->flush_upto = ticket; s->cv_launch.notify_one(); }     // its round launches now, whatever the policy
        while (s->completed_through < ticket) s->cv_done.wait(lk);
    }
    return s->err_code && ticket >= s->err_ticket ? s->err_code : MBLS_OK;
}

extern "C" int mbls_stream_query(mbls_stream* s, uint64_t ticket) {
    if (!s) return MBLS_ERR_ARGUMENT;
    std::lock_guard<std::mutex> g(s->mu);
    if (!ticket || ticket > s->last_ticket) return fail(s, MBLS_ERR_ARGUMENT, "unknown ticket %llu", (unsigned long long)ticket);
    if (s->completed_through < ticket) return MBLS_PENDING;
    return s->err_code && ticket >= s->err_ticket ? s->err_code : MBLS_OK;
}

extern "C" int mbls_stream_get_stats(mbls_stream* s, mbls_stream_stats* out) {
    if (!s || !out) return MBLS_ERR_ARGUMENT;
    std::lock_guard<std::mutex> g(s->mu);
    *out = s->stats;
    return MBLS_OK;
}

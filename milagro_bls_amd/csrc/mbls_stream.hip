// mbls_stream.hip -- the verification stream (include/mbls.h, "verification stream"): calls of any size in, full-round launches of the
// public device entries out. Built on the public ABI only: mbls_ctx_get_limits, mbls_ctx_reserve[_keys], mbls_plan_workspace_items and the
// three *_device verification entries (a message-table stream: their `_msgtable_device` forms), so every result comes out of the same verify_pipeline the parity
// tests pin. One hook below the ABI, not exported from the library: a message table counts the calls its streams hold (mblsi_msgtable_stream_calls), which mbls_msgtable_clear consults.
//
// A stream has ONE KIND, fixed at creation (stream_kind, mbls_stream_plan.h), and what differs between kinds stands in one place per question, as one switch:
//   what a call's arrays are, and who may submit it      submit / submit_cmt / submit_vm, refused for another kind by wrong_kind
//   whether a call may be split                          stream_kind_whole -> stream_step (mbls_stream.h), the one step absorb and both mbls_stream_cut* take
//   which slot buffers exist, how large                  slot_buffers
//   what the kind reserves in the context and its table  reserve_for_kind
//   what a round looks like (tiles, host copies, tables) stream_plan_keys / _committee / _vm (mbls_stream_plan.h), bounded by meta_capacity
//   which entry a round calls                            run_entry
//   how answers reach a host caller                      answer_host_piece
// KEYS (mbls_stream_create[_msgtable]): byte keys or key-table indices, message bytes or message-table indices; gathered by k_stream_gather, byte segment by byte
// segment. COMMITTEE (mbls_stream_create_committee): mbls_fast_aggregate_verify_batch_committee_msgtable_device over the slot; device pieces are staged by
// k_stream_gather_cmt, which re-strides every call's bitfields to the stream's stride, and the table is held by two more hooks (mblsi_committees_stream_*).
// VM (mbls_stream_create_vm_committee): whole verify_multiple batches, never split; a round is ONE call of
// mbls_verify_multiple_batches_committee_msgtable_locate_device over the slot with the ragged batch table of the plan, staged by k_stream_gather_vm and answered
// per call and per set by k_stream_scatter_vm; one more hook reserves that entry's own staging (mblsi_vbg_reserve_staging).
//
// Per stream: depth + 1 staging SLOTS (one round each: the open one and up to depth launched), one LAUNCHER thread that cuts the queue of submitted calls into the
// open slot (absorb), makes the round's plan and issues it (launch_round, the only launch function: gather on the stream's gather stream, the device entry and the
// scatter on its main HIP stream, a blocking-sync event behind them), and one COMPLETER thread that waits on those events in order, copies host results out of the
// pinned result areas, advances completed_through and frees the slot. Neither thread calls into the context with the stream's lock held; no HIP call is made from
// a host callback.
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
#include "mbls_stream_plan.h"

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

struct call_rec : stream_call {
    uint64_t ticket = 0; bool split = false;
    hipEvent_t ev = nullptr;                                                 // device submits: recorded on the caller's stream
};
struct piece_rec { std::shared_ptr<call_rec> c; uint64_t first, items, round_first; uint64_t batch = 0; };   // batch: a verify_multiple call's batch of the round

// a slot's buffers: the round's arrays on the device (dev[RA_*]; RA_KEYS holds a committee or verify_multiple round's fields), its results and the meta area, and
// in pinned memory the meta area, the results of host pieces and the mirrors the kind stages host pieces through (pin[RA_*]; slot_buffers says which exist)
struct slot {
    uint8_t* dev[RA_COUNT] = {}; uint8_t* pin[RA_COUNT] = {};
    uint8_t *d_res = nullptr, *d_meta = nullptr; uint32_t* d_st = nullptr;
    uint8_t *h_meta = nullptr, *h_res = nullptr; uint32_t* h_st = nullptr;
    hipEvent_t gev = nullptr, done = nullptr;
    std::vector<piece_rec> pieces;
    mbls_stream_fill fill{};
    stream_round_plan plan;
    bool full = false;
    uint64_t first_ticket = 0, done_through = 0;
    int rc = MBLS_OK;
};

}  // namespace

struct mbls_stream {
    mbls_ctx* ctx = nullptr; const mbls_keytable* tab = nullptr;
    stream_consts k{};                               // the kind, fixed at creation, and the constants a round's plan reads (k.o: the options with their defaults filled in)
    mbls_msgtable* mt = nullptr;                     // the message table of a committee or verify_multiple stream; on a keys stream non-null means a call's "message bytes" are its uint32 table indices (msg_len = 4)
    mbls_committees* cm = nullptr;                   // the committee table of a committee or verify_multiple stream, set once it is bound to k.bits_stride (until free_stream)
    int mode = 0, fmt = MBLS_PK_UNCOMPRESSED, dev = 0;
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

// the public entry a round of this kind is: one call over the slot's arrays, dense in round order (lock not held)
int run_entry(mbls_stream* s, slot& sl, const stream_round_plan& r) {
    const uint64_t n = r.n;
    uint8_t* const d_sigs = sl.dev[RA_SIGS]; uint8_t* const d_msgs = sl.dev[RA_MSGS]; uint8_t* const d_keys = sl.dev[RA_KEYS];
    const uint32_t* d_midx = (const uint32_t*)d_msgs; const uint32_t* d_cid = (const uint32_t*)sl.dev[RA_CID];
    int rc;
    switch (s->k.kind) {
        case STREAM_KEYS: {
            const uint64_t* d_moff = r.lay.msgs_uniform ? nullptr : (const uint64_t*)(sl.d_meta + r.at_m);
            const uint32_t* d_pkoff = r.lay.keys_uniform ? nullptr : (const uint32_t*)(sl.d_meta + r.at_k);
            const uint32_t msg_len = r.lay.msgs_uniform ? r.lay.msg_len : 0, k = r.lay.keys_uniform ? r.lay.k : 0;
            const bool verify = s->mode == MBLS_STREAM_VERIFY;
            // a message table: the staged "message bytes" are the items' table indices, dense in round order (every call has msg_len = 4 and no offsets)
            if (s->mt && verify) rc = mbls_verify_batch_msgtable_device(s->ctx, d_sigs, s->mt, d_midx, d_keys, s->fmt, n, sl.d_res, nullptr, sl.d_st, s->hs);
            else if (s->mt && s->tab)
                rc = mbls_fast_aggregate_verify_batch_indexed_msgtable_device(s->ctx, s->tab, d_sigs, s->mt, d_midx, (const uint32_t*)d_keys, d_pkoff, n, k, sl.d_res, nullptr, sl.d_st, s->hs);
            else if (s->mt) rc = mbls_fast_aggregate_verify_batch_msgtable_device(s->ctx, d_sigs, s->mt, d_midx, d_keys, s->fmt, d_pkoff, n, k, sl.d_res, nullptr, sl.d_st, s->hs);
            else if (verify) rc = mbls_verify_batch_device(s->ctx, d_sigs, d_msgs, msg_len, d_moff, d_keys, s->fmt, n, sl.d_res, nullptr, sl.d_st, s->hs);
            else if (s->tab)
                rc = mbls_fast_aggregate_verify_batch_indexed_device(s->ctx, s->tab, d_sigs, d_msgs, msg_len, d_moff, (const uint32_t*)d_keys, d_pkoff, n, k, sl.d_res, nullptr, sl.d_st, s->hs);
            else rc = mbls_fast_aggregate_verify_batch_device(s->ctx, d_sigs, d_msgs, msg_len, d_moff, d_keys, s->fmt, d_pkoff, n, k, sl.d_res, nullptr, sl.d_st, s->hs);
            break;
        }
        case STREAM_COMMITTEE:
            rc = mbls_fast_aggregate_verify_batch_committee_msgtable_device(s->ctx, s->cm, d_sigs, s->mt, d_midx, d_cid, d_keys, s->k.bits_stride, n, sl.d_res, nullptr, sl.d_st, s->hs);
            break;
        default:    // STREAM_VM: the batches entry with the ragged table of the meta area; the batches' bytes and words behind the sets'
            rc = mbls_verify_multiple_batches_committee_msgtable_locate_device(s->ctx, s->cm, d_sigs, d_cid, d_keys, s->k.bits_stride, s->mt, d_midx, (const uint64_t*)sl.dev[RA_RANDS], n,
                                                                               (const uint32_t*)(sl.d_meta + r.at_k), 0, r.batches, r.max_groups, sl.d_res + n, sl.d_st + n,
                                                                               sl.d_res, sl.d_st, s->hs);
            if (rc) return fail(s, rc, "round of %llu sets in %llu batches: %s", (unsigned long long)n, (unsigned long long)r.batches, mbls_last_error(s->ctx));
    }
    if (rc) return fail(s, rc, "round of %llu items: %s", (unsigned long long)n, mbls_last_error(s->ctx));
    return MBLS_OK;
}

// The round in the open slot: its plan (mbls_stream_plan.h), then the plan issued. On the gather stream the waits on the callers' events and the host copies in
// piece order, the one meta upload, the gather kernel of every tile list the plan filled, gev; on the main stream the wait on gev, the entry, the scatter kernel,
// the two result copies if a piece was a host piece, the completion event. Runs on the launcher thread without the stream's lock.
int launch_round(mbls_stream* s, slot& sl) {
    stream_round_plan& r = sl.plan;
    stream_plan(s->k, sl.pieces.data(), sl.pieces.size(), sl.dev, r);
    if (r.bytes > s->meta_bytes)
        return fail(s, MBLS_ERR_DEVICE, "internal: round meta of %llu bytes exceeds the slot's %llu", (unsigned long long)r.bytes, (unsigned long long)s->meta_bytes);
    stream_plan_pack(r, sl.h_meta);
    hipError_t e = hipSuccess;
    hipEvent_t last_ev = nullptr;
    size_t h = 0;
    for (size_t i = 0; i <= sl.pieces.size(); i++) {
        for (; h < r.hc.size() && r.hc[h].piece == i; h++) {
            const stream_hcopy& c = r.hc[h];
            uint8_t* const pinned = sl.pin[c.arr] + c.at;
            switch (c.how) {
                case HC_STAGE: memcpy(pinned, c.src, c.bytes); break;
                case HC_WIDEN: stream_widen(pinned, c.src, c.items, c.len, c.bytes / c.items); break;
                default:
                    if (e == hipSuccess) e = hipMemcpyAsync(sl.dev[c.arr] + c.at, c.how == HC_UPLOAD ? pinned : c.src, c.bytes, hipMemcpyHostToDevice, s->gs);
            }
        }
        if (i == sl.pieces.size()) break;
        const call_rec& c = *sl.pieces[i].c;
        if (!c.host && c.ev != last_ev) { if (e == hipSuccess) e = hipStreamWaitEvent(s->gs, c.ev, 0); last_ev = c.ev; }
    }
    if (e == hipSuccess && r.bytes) e = hipMemcpyAsync(sl.d_meta, sl.h_meta, r.bytes, hipMemcpyHostToDevice, s->gs);
    if (e == hipSuccess && !r.gt.empty()) { hipLaunchKernelGGL(k_stream_gather, dim3((unsigned)r.gt.size()), dim3(SWG), 0, s->gs, (const gtile*)(sl.d_meta + r.at_g)); e = hipGetLastError(); }
    if (e == hipSuccess && !r.ct.empty()) {
        hipLaunchKernelGGL(k_stream_gather_cmt, dim3((unsigned)r.ct.size()), dim3(SWG), 0, s->gs, (const ctile*)(sl.d_meta + r.at_c), sl.dev[RA_SIGS], (uint32_t*)sl.dev[RA_MSGS],
                           (uint32_t*)sl.dev[RA_CID], sl.dev[RA_KEYS], s->k.bits_stride);
        e = hipGetLastError();
    }
    if (e == hipSuccess && !r.vt.empty()) {
        hipLaunchKernelGGL(k_stream_gather_vm, dim3((unsigned)r.vt.size()), dim3(SWG), 0, s->gs, (const vtile*)(sl.d_meta + r.at_g), sl.dev[RA_SIGS], (uint32_t*)sl.dev[RA_CID], sl.dev[RA_KEYS],
                           (uint32_t*)sl.dev[RA_MSGS], (uint64_t*)sl.dev[RA_RANDS], s->k.bits_stride);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(sl.gev, s->gs);
    if (e == hipSuccess) e = hipStreamWaitEvent(s->hs, sl.gev, 0);
    if (e != hipSuccess) return fail(s, MBLS_ERR_DEVICE, "gather: %s", hipGetErrorString(e));
    const int rc = run_entry(s, sl, r);
    if (rc) return rc;
    const uint64_t answers = r.n + r.batches;
    if (!r.st.empty()) { hipLaunchKernelGGL(k_stream_scatter, dim3((unsigned)r.st.size()), dim3(SWG), 0, s->hs, (const stile*)(sl.d_meta + r.at_s), (const uint8_t*)sl.d_res, (const uint32_t*)sl.d_st); e = hipGetLastError(); }
    if (!r.vst.empty()) { hipLaunchKernelGGL(k_stream_scatter_vm, dim3((unsigned)r.vst.size()), dim3(SWG), 0, s->hs, (const vstile*)(sl.d_meta + r.at_s), (const uint8_t*)sl.d_res, (const uint32_t*)sl.d_st); e = hipGetLastError(); }
    if (e == hipSuccess && r.any_host) e = hipMemcpyAsync(sl.h_res, sl.d_res, answers, hipMemcpyDeviceToHost, s->hs);
    if (e == hipSuccess && r.any_host) e = hipMemcpyAsync(sl.h_st, sl.d_st, 4 * answers, hipMemcpyDeviceToHost, s->hs);
    if (e == hipSuccess) e = hipEventRecord(sl.done, s->hs);
    if (e != hipSuccess) return fail(s, MBLS_ERR_DEVICE, "scatter: %s", hipGetErrorString(e));
    std::lock_guard<std::mutex> g(s->mu);
    s->stats.gathered_bytes += r.gathered;
    return MBLS_OK;
}

// cut queued calls into the open slot (lock held): the step mbls_stream_cut and mbls_stream_cut_vm run (stream_step), a flush boundary after call flush_upto
void absorb(mbls_stream* s, slot& sl) {
    while (s->cursor <= s->last_ticket && !sl.full) {
        const std::shared_ptr<call_rec>& c = s->calls[s->cursor - s->base];
        if (sl.fill.items && sl.first_ticket <= s->flush_upto && c->ticket > s->flush_upto) break;
        const mbls_stream_step st = stream_step(s->k.o, stream_kind_whole(s->k.kind), sl.fill, c->shape, s->item_off);
        if (st.items) {
            if (sl.pieces.empty()) sl.first_ticket = c->ticket;
            if (s->item_off) c->split = true;
            sl.pieces.push_back(piece_rec{c, s->item_off, st.items, st.round_first, st.batch});
            s->item_off += st.items;
        }
        if (s->item_off == c->shape.n) { sl.done_through = c->ticket; s->cursor++; s->item_off = 0; }
        sl.full = st.full;
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
            o.pieces.clear(); o.fill = mbls_stream_fill{}; o.full = false; o.first_ticket = 0; o.done_through = s->cut_done_through; o.rc = MBLS_OK;
        }
        slot& o = s->slots[s->open];
        absorb(s, o);
        const bool flush = o.fill.items && o.first_ticket <= s->flush_upto;
        const bool wc = s->k.o.policy == MBLS_STREAM_WORK_CONSERVING && s->inflight.size() < s->k.o.depth;
        if (o.fill.items && (o.full || flush || wc)) {
            const int si = s->open; s->open = -1;
            s->cut_done_through = o.done_through;
            s->stats.rounds++; s->stats.full_rounds += o.full; s->stats.pieces += o.pieces.size();
            for (const piece_rec& p : o.pieces) if (p.first && p.c->split && p.first + p.items == p.c->shape.n) s->stats.split_calls++;
            const bool dead = s->dead;
            lk.unlock();
            int rc = dead ? MBLS_ERR_DEVICE : launch_round(s, o);
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

// a completed round's answers to a host piece, from the slot's pinned result areas (lock not held)
void answer_host_piece(const mbls_stream* s, const slot& sl, const piece_rec& p) {
    const call_rec& c = *p.c;
    switch (s->k.kind) {
        case STREAM_VM: {     // the call's batch byte and word (kept behind the round's sets), then its sets'
            const uint64_t at = sl.plan.n + p.batch;
            c.res[0] = sl.h_res[at];
            if (c.st) c.st[0] = sl.h_st[at];
            if (c.set_res) memcpy(c.set_res, sl.h_res + p.round_first, p.items);
            if (c.set_st) memcpy(c.set_st, sl.h_st + p.round_first, 4 * p.items);
            break;
        }
        default:              // one byte and word per item, at the piece's place in the call
            memcpy(c.res + p.first, sl.h_res + p.round_first, p.items);
            if (c.st) memcpy(c.st + p.first, sl.h_st + p.round_first, 4 * p.items);
    }
}

// the tables' counts of the calls this stream holds (the handles a kind does not have are null)
void count_calls(mbls_stream* s, long long delta) {
    if (s->mt) mblsi_msgtable_stream_calls(s->mt, delta);
    if (s->cm) mblsi_committees_stream_calls(s->cm, delta);
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
            for (const piece_rec& p : sl.pieces) if (p.c->host) answer_host_piece(s, sl, p);
        lk.lock();
        if (rc) {
            s->dead = true;
            if (!s->err_code) { s->err_code = rc; s->err_ticket = sl.first_ticket; }
        }
        if (sl.done_through > s->completed_through) s->completed_through = sl.done_through;
        sl.pieces.clear();
        while (!s->calls.empty() && s->calls.front()->ticket <= s->completed_through && s->calls.front()->ticket < s->cursor) {
            if (s->calls.front()->ev) s->ev_pool.push_back(s->calls.front()->ev);
            count_calls(s, -1);
            s->calls.pop_front(); s->base++;
        }
        s->inflight.pop_front(); s->free_slots.push_back(si);
        s->cv_launch.notify_one(); s->cv_done.notify_all();
    }
}

// Every buffer of a slot of this stream, in the order they are allocated: where its pointer is kept, device or pinned memory, bytes. Everything is allocated at
// creation (alloc_slot) and freed from the same list (free_stream). R items of 96 signature bytes; a keys round holds round_msg_bytes of messages and
// round_keys keys of `unit` bytes; a committee or verify_multiple round holds R indices, ids and fields of bits_stride bytes, and the fields of host pieces pass
// through pinned memory; a verify_multiple round also holds R scalars, and ONE pinned block mirrors its host calls' other four arrays (alloc_slot carves it).
struct slot_buf { const char* name; void** p; bool pinned; uint64_t bytes; };
constexpr size_t SLOT_BUFS = 16;
size_t slot_buffers(const stream_consts& k, uint64_t meta_bytes, slot& sl, slot_buf* b) {
    const uint64_t R = k.o.round_items, fields = std::max<uint64_t>((uint64_t)k.bits_stride * R, 16);
    size_t n = 0;
    auto dev = [&](const char* name, void* p, uint64_t bytes) { b[n++] = slot_buf{name, (void**)p, false, bytes}; };
    auto pin = [&](const char* name, void* p, uint64_t bytes) { b[n++] = slot_buf{name, (void**)p, true, bytes}; };
    dev("signatures", &sl.dev[RA_SIGS], 96 * R);
    switch (k.kind) {
        case STREAM_KEYS:
            dev("messages", &sl.dev[RA_MSGS], std::max<uint64_t>(k.o.round_msg_bytes, 16));
            dev("keys", &sl.dev[RA_KEYS], std::max<uint64_t>(k.unit * k.o.round_keys, 16));
            break;
        case STREAM_COMMITTEE:
            dev("message indices", &sl.dev[RA_MSGS], std::max<uint64_t>(k.o.round_msg_bytes, 16));
            dev("fields", &sl.dev[RA_KEYS], fields); dev("committee ids", &sl.dev[RA_CID], 4 * R); pin("host fields", &sl.pin[RA_KEYS], fields);
            break;
        default:    // STREAM_VM; the mirror: signatures | scalars | set words | message indices, each at its alignment
            dev("message indices", &sl.dev[RA_MSGS], std::max<uint64_t>(4 * R, 16));
            dev("scalars", &sl.dev[RA_RANDS], 8 * R); pin("host mirror", &sl.pin[RA_SIGS], (96 + 8 + 4 + 4) * R);
            dev("fields", &sl.dev[RA_KEYS], fields); dev("set words", &sl.dev[RA_CID], 4 * R); pin("host fields", &sl.pin[RA_KEYS], fields);
    }
    dev("results", &sl.d_res, R); dev("status", &sl.d_st, 4 * R); dev("meta", &sl.d_meta, meta_bytes);
    pin("host meta", &sl.h_meta, meta_bytes); pin("host results", &sl.h_res, R); pin("host status", &sl.h_st, 4 * R);
    return n;
}

hipError_t alloc_slot(const mbls_stream* s, slot& sl) {
    slot_buf b[SLOT_BUFS]; const size_t nb = slot_buffers(s->k, s->meta_bytes, sl, b);
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < nb && e == hipSuccess; i++) e = b[i].pinned ? hipHostMalloc(b[i].p, b[i].bytes, hipHostMallocDefault) : hipMalloc(b[i].p, b[i].bytes);
    if (e == hipSuccess && s->k.kind == STREAM_VM) {
        const uint64_t R = s->k.o.round_items;
        sl.pin[RA_RANDS] = sl.pin[RA_SIGS] + 96 * R; sl.pin[RA_CID] = sl.pin[RA_RANDS] + 8 * R; sl.pin[RA_MSGS] = sl.pin[RA_CID] + 4 * R;
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.gev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming | hipEventBlockingSync);
    return e;
}

void free_stream(mbls_stream* s) {
    for (slot& sl : s->slots) {
        slot_buf b[SLOT_BUFS]; const size_t nb = slot_buffers(s->k, s->meta_bytes, sl, b);
        for (size_t i = 0; i < nb; i++) if (*b[i].p) (void)(b[i].pinned ? hipHostFree(*b[i].p) : hipFree(*b[i].p));
        if (sl.gev) (void)hipEventDestroy(sl.gev);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    for (hipEvent_t ev : s->ev_pool) (void)hipEventDestroy(ev);
    for (auto& c : s->calls) if (c->ev) (void)hipEventDestroy(c->ev);
    if (s->hs) (void)hipStreamDestroy(s->hs);
    if (s->gs) (void)hipStreamDestroy(s->gs);
    if (s->cm) mblsi_committees_stream_unbind(s->cm, s->k.bits_stride);      // (set once the table was bound to the stride)
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
    count_calls(s, 1);
    s->stats.calls++; s->stats.items += n;
    *ticket = c->ticket;
    s->cv_launch.notify_one();
    return MBLS_OK;
}

// the four families of submit entries, and what each is told on a stream that does not take its calls (nullptr: this stream does)
enum submit_via { VIA_BYTES, VIA_MSGIDX, VIA_COMMITTEE, VIA_VM };
const char* wrong_kind(const mbls_stream* s, submit_via via) {
    const int kind = s->k.kind;
    switch (via) {
        case VIA_BYTES:
        case VIA_MSGIDX:
            if (kind == STREAM_VM) return "a verify_multiple stream takes whole batches of sets (mbls_stream_submit_vm[_device])";
            if (kind == STREAM_COMMITTEE) return "a committee stream takes committee ids and bitfields (mbls_stream_submit_committee[_device])";
            if ((via == VIA_MSGIDX) == (s->mt != nullptr)) return nullptr;
            return s->mt ? "a message-table stream takes message indices (mbls_stream_submit_msgidx[_device])"
                         : "this stream takes messages, not message-table indices (mbls_stream_submit[_device])";
        case VIA_COMMITTEE:
            if (kind == STREAM_COMMITTEE) return nullptr;
            if (kind == STREAM_VM) return "a verify_multiple stream takes whole batches of sets (mbls_stream_submit_vm[_device])";
            return s->mt ? "this is not a committee stream: a message-table stream takes mbls_stream_submit_msgidx[_device]"
                         : "this is not a committee stream: it takes messages and keys (mbls_stream_submit[_device])";
        default:
            if (kind == STREAM_VM) return nullptr;
            if (kind == STREAM_COMMITTEE) return "this is not a verify_multiple stream: a committee stream takes mbls_stream_submit_committee[_device]";
            return s->mt ? "this is not a verify_multiple stream: a message-table stream takes mbls_stream_submit_msgidx[_device]"
                         : "this is not a verify_multiple stream: it takes messages and keys (mbls_stream_submit[_device])";
    }
}
// what every submit checks first; 0: go on
int refuse_early(mbls_stream* s, submit_via via, const uint64_t* ticket) {
    if (!s) return MBLS_ERR_ARGUMENT;
    if (!ticket) return fail(s, MBLS_ERR_ARGUMENT, "null ticket pointer");
    const char* why = wrong_kind(s, via);
    return why ? fail(s, MBLS_ERR_ARGUMENT, "%s", why) : 0;
}

int submit(mbls_stream* s, bool msgidx, bool host, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* moff, const uint8_t* pks,
           const uint32_t* idx, const uint32_t* poff, uint64_t n, uint32_t k, uint8_t* res, uint64_t* bm, uint32_t* st, void* stream, uint64_t* ticket) {
    if (const int rc = refuse_early(s, msgidx ? VIA_MSGIDX : VIA_BYTES, ticket)) return rc;
    if (n == 0) return fail(s, MBLS_ERR_ARGUMENT, "a call holds at least one item");
    if (!sigs || !res) return fail(s, MBLS_ERR_ARGUMENT, "null buffer");
    if (s->mode == MBLS_STREAM_VERIFY && (poff || k != 1)) return fail(s, MBLS_ERR_ARGUMENT, "verify mode: one key per item (k = 1, no key offsets)");
    if (s->tab ? pks != nullptr : idx != nullptr)
        return fail(s, MBLS_ERR_ARGUMENT, s->tab ? "an index stream takes key indices, not key bytes" : "a byte-key stream takes key bytes, not key indices");
    const mbls_stream_opts& o = s->k.o;
    mbls_stream_call_shape sh{n, k, msg_len, poff, moff, 0};
    int what = 0; const uint64_t bad = stream_check_call(o, sh, &what);
    if (bad) {
        const uint64_t i = bad - 1;
        if (what == 1) return fail(s, MBLS_ERR_ARGUMENT, "offset table runs backwards (or holds a message of 2^32 bytes or more) at item %llu", (unsigned long long)i);
        if (what == 2) return fail(s, MBLS_ERR_ARGUMENT, "item %llu has %llu keys; a round holds %llu (mbls_stream_opts.round_keys)", (unsigned long long)i,
                                   (unsigned long long)stream_item_keys(sh, i), (unsigned long long)o.round_keys);
        return fail(s, MBLS_ERR_ARGUMENT, "item %llu has a %llu-byte message; a round holds %llu message bytes (mbls_stream_opts.round_msg_bytes)", (unsigned long long)i,
                    (unsigned long long)stream_item_msg(sh, i), (unsigned long long)o.round_msg_bytes);
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
    if (const int rc = refuse_early(s, VIA_COMMITTEE, ticket)) return rc;
    if (n == 0) return fail(s, MBLS_ERR_ARGUMENT, "a call holds at least one item");
    if (!sigs || !res || !msg_idx || !cmt_idx || !bits) return fail(s, MBLS_ERR_ARGUMENT, "null buffer");
    if (bits_len == 0 || bits_len > s->k.bits_stride)
        return fail(s, MBLS_ERR_ARGUMENT, "bits_len is %u; a field holds 1 to %u bytes (the stream's bits_stride)", bits_len, s->k.bits_stride);
    mbls_stream_call_shape sh{n, 0, 4, nullptr, nullptr, 0};
    int what = 0;
    if (stream_check_call(s->k.o, sh, &what))
        return fail(s, MBLS_ERR_ARGUMENT, "an item takes 4 message bytes; a round holds %llu (mbls_stream_opts.round_msg_bytes)", (unsigned long long)s->k.o.round_msg_bytes);
    auto c = std::make_shared<call_rec>();
    c->host = host; c->shape = sh; c->sigs = sigs; c->msgs = (const uint8_t*)msg_idx; c->keys = (const uint8_t*)cmt_idx; c->bits = bits; c->bits_len = bits_len;
    c->res = res; c->bm = bm; c->st = st;
    return enqueue(s, c, stream, ticket);
}

// a verify_multiple call: one batch of n sets, never split (shape.n = its sets; the cutting reads nothing else of the shape)
int submit_vm(mbls_stream* s, bool host, const uint8_t* sigs, const uint32_t* cmt_idx, const uint8_t* bits, uint32_t bits_len, const uint32_t* msg_idx, const uint64_t* rands,
              uint64_t n, uint8_t* res, uint32_t* st, uint8_t* set_res, uint32_t* set_st, void* stream, uint64_t* ticket) {
    if (const int rc = refuse_early(s, VIA_VM, ticket)) return rc;
    if (n == 0) return fail(s, MBLS_ERR_ARGUMENT, "a call holds at least one set");
    if (!rands) return fail(s, MBLS_ERR_ARGUMENT, "verify_multiple without blinding scalars is forgeable: rands must not be NULL");
    if (!sigs || !res || !msg_idx || !cmt_idx) return fail(s, MBLS_ERR_ARGUMENT, "null buffer");
    if (bits_len > s->k.bits_stride) return fail(s, MBLS_ERR_ARGUMENT, "bits_len is %u; a field holds 0 to %u bytes (the stream's bits_stride)", bits_len, s->k.bits_stride);
    if (bits_len && !bits) return fail(s, MBLS_ERR_ARGUMENT, "null bitfields with bits_len = %u (only bits_len = 0 allows it)", bits_len);
    if (!stream_vm_fits(s->k.o, n))
        return fail(s, MBLS_ERR_ARGUMENT, "a call of %llu sets costs %llu of a round; a round holds %llu (mbls_stream_opts.round_items): at most %llu sets per call",
                    (unsigned long long)n, (unsigned long long)stream_vm_cost(n), (unsigned long long)s->k.o.round_items, (unsigned long long)(s->k.o.round_items - 1));
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

// the cut of a queue as data: every piece the walk (stream_walk) makes of calls shape(0 .. n_calls), under either rule
template <typename Shape>
int cut_queue(const mbls_stream_opts& o, int whole, uint64_t n_calls, Shape shape, mbls_stream_piece* out, uint64_t max_pieces, uint64_t* n_pieces) {
    uint64_t np = 0;
    stream_walk(o, whole, n_calls, shape, [&](uint64_t j, uint64_t first, const mbls_stream_step& st, uint64_t round, const mbls_stream_fill&) {
        if (np < max_pieces) out[np] = mbls_stream_piece{j, first, st.items, round, st.round_first};
        np++;
    });
    *n_pieces = np;
    return np <= max_pieces || !out ? MBLS_OK : MBLS_ERR_ARGUMENT;
}

}  // namespace

extern "C" int mbls_stream_cut_vm(const mbls_stream_opts* o, const uint64_t* call_sets, const uint32_t* flush_after, uint64_t n_calls, mbls_stream_piece* out,
                                  uint64_t max_pieces, uint64_t* n_pieces) {
    if (!o || !call_sets || !n_calls || !n_pieces || !o->round_items || (!out && max_pieces)) return MBLS_ERR_ARGUMENT;
    for (uint64_t j = 0; j < n_calls; j++) if (!stream_vm_fits(*o, call_sets[j])) return MBLS_ERR_ARGUMENT;
    auto shape = [&](uint64_t j) { return mbls_stream_call_shape{call_sets[j], 0, 4, nullptr, nullptr, flush_after ? flush_after[j] : 0u}; };
    return cut_queue(*o, 1, n_calls, shape, out, max_pieces, n_pieces);
}

extern "C" int mbls_stream_cut(const mbls_stream_opts* o, const mbls_stream_call_shape* calls, uint64_t n_calls, mbls_stream_piece* out, uint64_t max_pieces,
                               uint64_t* n_pieces) {
    if (!o || !calls || !n_calls || !n_pieces || !o->round_items || !o->round_keys || !o->round_msg_bytes || (!out && max_pieces)) return MBLS_ERR_ARGUMENT;
    for (uint64_t j = 0; j < n_calls; j++) {
        int what; if (!calls[j].n || stream_check_call(*o, calls[j], &what)) return MBLS_ERR_ARGUMENT;
    }
    return cut_queue(*o, 0, n_calls, [&](uint64_t j) { return calls[j]; }, out, max_pieces, n_pieces);
}

// What a stream of this kind takes hold of at creation: its committee table, bound to the stride (checked against this context, and from here on its appends
// against the stride; s->cm is set once bound, free_stream releases it), and in the context every round size's workspace up front, so that no round grows it.
static int reserve_for_kind(mbls_stream* s, const mbls_limits& L, mbls_committees* cm, bool compressed_keys) {
    const mbls_stream_opts& o = s->k.o;
    uint64_t ws = 0;
    // rounds of 1 .. round_items items (a partial round on the wave engine may take the eight-lane key sum, n + 8 n items)
    auto rounds_of_items = [&](bool committee) {
        const uint32_t kmax = (uint32_t)std::min<uint64_t>(o.round_keys, 0xFFFFFFFFull);
        for (uint64_t n = 1; n <= o.round_items; n++) {
            ws = std::max(ws, mbls_plan_workspace_items(&L, n, kmax, 1));
            if (kmax >= 32) ws = std::max(ws, mbls_plan_workspace_items(&L, n, 32, 1));
            if (committee) ws = std::max(ws, mbls_plan_workspace_items(&L, n, 0, 0));
        }
    };
    auto bind = [&]() { const int rc = mblsi_committees_stream_bind(s->ctx, cm, s->k.bits_stride); if (!rc) s->cm = cm; return rc; };
    // the index lists k_cmt_expand writes for a full round of the largest committees the stride admits
    auto committee_items = [&]() { return mbls_ctx_reserve_committee_items(s->ctx, o.round_items, (uint32_t)std::min<uint64_t>(8ull * s->k.bits_stride, MBLS_COMMITTEE_MAX_MEMBERS)); };
    int rc;
    switch (s->k.kind) {
        case STREAM_KEYS:
            rounds_of_items(false);
            rc = mbls_ctx_reserve(s->ctx, ws);                    // (leaves the context's device current on this thread)
            if (!rc && compressed_keys) rc = mbls_ctx_reserve_keys(s->ctx, o.round_keys);
            return rc;
        case STREAM_COMMITTEE:
            if ((rc = bind())) return rc;
            rounds_of_items(true);
            rc = mbls_ctx_reserve(s->ctx, ws);
            return rc ? rc : committee_items();
        default:    // STREAM_VM
            if ((rc = bind())) return rc;
            // a verify_multiple round holds B batches of n sets in all with n + B <= round_items and B <= n. What the batches entry reserves
            // (mbls_plan_verify_multiple_batches_committee) does not decrease in n, in B or in the bound on the groups, and the bound is at most n: so the largest of
            // every (n, B) a round can hold lies on n = round_items - B, with no promise on the groups and a table that caps nothing, on either route, with locate
            for (uint64_t B = 1; 2 * B <= o.round_items; B++)
                for (int route = 1; route <= 2; route++) {
                    mbls_vm_batches_committee_plan vp;
                    if (!mbls_plan_verify_multiple_batches_committee(&L, o.round_items - B, B, 0, 0xFFFFFFFFull, 0, route, 1, &vp)) ws = std::max(ws, vp.workspace_items);
                }
            rc = mbls_ctx_reserve(s->ctx, ws);
            if (!rc) rc = committee_items();
            // the batches entry's own grow-only staging: the set map of a ragged batch table and the group arrays, for the most sets and batches a round holds
            if (!rc) rc = mblsi_vbg_reserve_staging(s->ctx, o.round_items - 1, o.round_items / 2);
            return rc;
    }
}

static int stream_create(mbls_ctx* ctx, int kind, int mode, int pk_format, const mbls_keytable* t, mbls_msgtable* mt, mbls_committees* cm, uint32_t bits_stride,
                         const mbls_stream_opts* opts, mbls_stream** out) {
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
    if (stream_kind_whole(kind) && o.round_items < 2) return MBLS_ERR_ARGUMENT;   // the smallest whole call, one set and its signature pair, costs 2
    mbls_stream* s = new (std::nothrow) mbls_stream();
    if (!s) return MBLS_ERR_DEVICE;
    s->ctx = ctx; s->tab = t; s->mt = mt; s->mode = mode; s->fmt = t ? MBLS_PK_UNCOMPRESSED : pk_format;
    s->k = stream_consts{kind, mode == MBLS_STREAM_VERIFY, kind != STREAM_KEYS ? 0u : t ? 4u : (pk_format == MBLS_PK_COMPRESSED ? 48u : 96u), bits_stride, o};
    rc = reserve_for_kind(s, L, cm, !t && pk_format == MBLS_PK_COMPRESSED);
    if (rc) { free_stream(s); return rc; }
    hipError_t e = hipGetDevice(&s->dev);
    s->meta_bytes = meta_capacity(s->k);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->hs, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->gs, hipStreamNonBlocking);
    s->slots.resize(o.depth + 1);
    for (slot& sl : s->slots) if (e == hipSuccess) e = alloc_slot(s, sl);
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
    return stream_create(ctx, STREAM_KEYS, mode, pk_format, t, nullptr, nullptr, 0, opts, out);
}
extern "C" int mbls_stream_create_msgtable(mbls_ctx* ctx, int mode, int pk_format, const mbls_keytable* t, mbls_msgtable* mt, const mbls_stream_opts* opts, mbls_stream** out) {
    if (!mt) return MBLS_ERR_ARGUMENT;
    return stream_create(ctx, STREAM_KEYS, mode, pk_format, t, mt, nullptr, 0, opts, out);
}
// a committee stream: fast_aggregate_verify over the committee table (and through it its key table) and the message table
extern "C" int mbls_stream_create_committee(mbls_ctx* ctx, mbls_committees* committees, mbls_msgtable* mt, uint32_t bits_stride, const mbls_stream_opts* opts,
                                            mbls_stream** out) {
    if (!committees || !mt) return MBLS_ERR_ARGUMENT;
    return stream_create(ctx, STREAM_COMMITTEE, MBLS_STREAM_FAST_AGGREGATE_VERIFY, MBLS_PK_UNCOMPRESSED, nullptr, mt, committees, bits_stride, opts, out);
}
// a verify_multiple stream over the same two tables: a call is a batch, a round one call of mbls_verify_multiple_batches_committee_msgtable_locate_device
extern "C" int mbls_stream_create_vm_committee(mbls_ctx* ctx, mbls_committees* committees, mbls_msgtable* mt, uint32_t bits_stride, const mbls_stream_opts* opts,
                                               mbls_stream** out) {
    if (!committees || !mt) return MBLS_ERR_ARGUMENT;
    return stream_create(ctx, STREAM_VM, MBLS_STREAM_FAST_AGGREGATE_VERIFY, MBLS_PK_UNCOMPRESSED, nullptr, mt, committees, bits_stride, opts, out);
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

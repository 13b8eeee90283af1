// mbls_stream.h -- the pure parts of the verification stream (include/mbls.h, "verification stream"), in a header of their own so that a
// host compiler can build them for the CPU tests (tests/host_emul/mbls_stream_harness.cpp): the cutting rule that packs calls into rounds,
// the layout decision of a round, the bit arithmetic of the scatter into a caller's bitmap, and one destination dword of a committee call's re-strided bitfield
// (tests/stream_cmt_emul/mbls_stream_cmt_harness.cpp), and the whole-call rule and the batch table of a verify_multiple stream
// (tests/stream_vm_emul/mbls_stream_vm_harness.cpp), and the one step and walk over a queue of calls that both rules are reached through. mbls_stream.hip runs
// exactly these; what a round looks like once it is cut is mbls_stream_plan.h.
#ifndef MBLS_STREAM_H
#define MBLS_STREAM_H
#include <stdint.h>
#include "../../include/mbls.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define MBLS_SFN static inline __host__ __device__
#else
#define MBLS_SFN static inline
#endif

// ---- cutting: the fill of the open round (its items, their keys and message bytes; on a stream of whole calls its sets and the calls they came in) and the
// largest run of a call's items that still fits it. cost: what of round_items is used -- the items, plus one per whole call; cost == items + calls at all
// times. The whole-call rule once kept a fill of its own: its type name and its name for the sets remain as aliases, so code written against it still builds.
struct mbls_stream_fill { union { uint64_t items, sets; }; uint64_t keys, msg_bytes, calls, cost; };
typedef mbls_stream_fill mbls_stream_vm_fill;

MBLS_SFN uint64_t stream_item_keys(const mbls_stream_call_shape& c, uint64_t i) { return c.pk_offsets ? (uint64_t)(c.pk_offsets[i + 1] - c.pk_offsets[i]) : c.k; }
MBLS_SFN uint64_t stream_item_msg(const mbls_stream_call_shape& c, uint64_t i) { return c.msg_offsets ? c.msg_offsets[i + 1] - c.msg_offsets[i] : c.msg_len; }

// items [first, first + return value) of call c join the open round (f is advanced past them); fewer than c.n - first means the next item does
// not fit: the round is full. Uniform calls take their run in one step, ragged ones item by item.
MBLS_SFN uint64_t stream_take(const mbls_stream_opts& o, mbls_stream_fill& f, const mbls_stream_call_shape& c, uint64_t first) {
    if (first >= c.n || f.items >= o.round_items) return 0;
    uint64_t t;
    if (!c.pk_offsets && !c.msg_offsets) {
        uint64_t room = o.round_items - f.items;
        if (c.k) { const uint64_t r = (o.round_keys - f.keys) / c.k; room = r < room ? r : room; }
        if (c.msg_len) { const uint64_t r = (o.round_msg_bytes - f.msg_bytes) / c.msg_len; room = r < room ? r : room; }
        t = c.n - first < room ? c.n - first : room;
        f.keys += t * c.k; f.msg_bytes += t * c.msg_len;
    } else {
        uint64_t i = first, keys = f.keys, msg = f.msg_bytes;
        const uint64_t end = first + (o.round_items - f.items) < c.n ? first + (o.round_items - f.items) : c.n;
        for (; i < end; i++) {
            const uint64_t ki = stream_item_keys(c, i), mi = stream_item_msg(c, i);
            if (keys + ki > o.round_keys || msg + mi > o.round_msg_bytes) break;
            keys += ki; msg += mi;
        }
        t = i - first; f.keys = keys; f.msg_bytes = msg;
    }
    f.items += t; f.cost += t;
    return t;
}

// ---- whole calls (a verify_multiple stream, mbls_stream_create_vm_committee): a call is ONE batch and a batch's verdict is one pairing product, so a call is
// never split. A call of n_sets sets costs n_sets + 1 of round_items -- its sets plus its signature pair, the Miller items of the per-set route, so that launch
// stays within a round. A call joins the open round when its cost fits what is left; otherwise it closes the round and opens the next one. A call that costs more
// than an empty round holds is refused at submit (stream_vm_fits). mbls_stream_cut_vm states this rule as data.
MBLS_SFN uint64_t stream_vm_cost(uint64_t n_sets) { return n_sets + 1; }
// what the round's calls cost together: its sets plus one per call
MBLS_SFN uint64_t stream_vm_used(const mbls_stream_fill& f) { return f.cost; }
MBLS_SFN int stream_vm_fits(const mbls_stream_opts& o, uint64_t n_sets) { return n_sets >= 1 && n_sets < o.round_items; }
// 1: the call joined the open round (f advanced: it is batch f.calls - 1 and its sets start at the old f.items); 0: it does not fit, the round is closed
MBLS_SFN int stream_take_whole(const mbls_stream_opts& o, mbls_stream_fill& f, uint64_t n_sets) {
    if (stream_vm_cost(n_sets) > o.round_items - stream_vm_used(f)) return 0;
    f.items += n_sets; f.calls++; f.cost += stream_vm_cost(n_sets);
    return 1;
}
// no further call fits: the smallest one costs 2
MBLS_SFN int stream_vm_full(const mbls_stream_opts& o, const mbls_stream_fill& f) { return o.round_items - stream_vm_used(f) < 2; }
// the ragged batch table of a round whose calls hold call_sets[0 .. n_calls) sets: off[0 .. n_calls], off[b] the first set of batch b, off[n_calls] the round's sets
MBLS_SFN void stream_vm_offsets(const uint64_t* call_sets, uint64_t n_calls, uint32_t* off) {
    uint64_t at = 0;
    for (uint64_t b = 0; b < n_calls; b++) { off[b] = (uint32_t)at; at += call_sets[b]; }
    off[n_calls] = (uint32_t)at;
}

// ---- the step every walk over a queue of calls takes, under either rule (`whole`: a stream of whole calls): call c is offered to the open round from its item
// `first` on. items: how many joined (a whole call: all or none), at round_first of the round, as batch `batch` of it (whole calls; 0 otherwise); full: the round
// is closed -- the rest of the call did not fit, or nothing more can join. The launcher (absorb), mbls_stream_cut and mbls_stream_cut_vm run this and nothing else.
struct mbls_stream_step { uint64_t items, round_first, batch; int full; };
MBLS_SFN mbls_stream_step stream_step(const mbls_stream_opts& o, int whole, mbls_stream_fill& f, const mbls_stream_call_shape& c, uint64_t first) {
    const uint64_t before = f.items;
    if (whole) {
        if (!stream_take_whole(o, f, c.n)) return mbls_stream_step{0, before, 0, 1};
        return mbls_stream_step{c.n, before, f.calls - 1, stream_vm_full(o, f)};
    }
    const uint64_t t = stream_take(o, f, c, first);
    return mbls_stream_step{t, before, 0, first + t < c.n || f.items == o.round_items};
}

// the walk over a whole queue: every call offered until all of it has joined, a full round followed by an empty one, a round closed behind a call whose
// flush_after is set. shape(j): call j; piece(j, first, step, round, fill): a piece and the fill it leaves. Returns the rounds, or -1 when a call joins no
// empty round (which the checks at submit exclude).
template <typename Shape, typename Piece>
static inline int64_t stream_walk(const mbls_stream_opts& o, int whole, uint64_t n_calls, Shape shape, Piece piece) {
    mbls_stream_fill f{}; uint64_t round = 0;
    for (uint64_t j = 0; j < n_calls; j++) {
        const mbls_stream_call_shape c = shape(j);
        for (uint64_t first = 0; first < c.n;) {
            const bool was_empty = !f.items;
            const mbls_stream_step st = stream_step(o, whole, f, c, first);
            if (!st.items && was_empty) return -1;
            if (st.items) { piece(j, first, st, round, (const mbls_stream_fill&)f); first += st.items; }
            if (st.full) { round++; f = mbls_stream_fill{}; }
        }
        if (c.flush_after && f.items) { round++; f = mbls_stream_fill{}; }
    }
    return (int64_t)(round + (f.items ? 1 : 0));
}

// the call as a whole: offsets non-decreasing (messages below 2^32 bytes, as the host entries require), and no item larger than an empty round.
// Returns 0, or 1 + the index of the first offending item with *what = 1 (offsets), 2 (keys), 3 (message bytes).
MBLS_SFN uint64_t stream_check_call(const mbls_stream_opts& o, const mbls_stream_call_shape& c, int* what) {
    for (uint64_t i = 0; i < c.n; i++) {
        if (c.pk_offsets && c.pk_offsets[i + 1] < c.pk_offsets[i]) { *what = 1; return i + 1; }
        if (c.msg_offsets && (c.msg_offsets[i + 1] < c.msg_offsets[i] || c.msg_offsets[i + 1] - c.msg_offsets[i] > 0xFFFFFFFFull)) { *what = 1; return i + 1; }
        if (stream_item_keys(c, i) > o.round_keys) { *what = 2; return i + 1; }
        if (stream_item_msg(c, i) > o.round_msg_bytes) { *what = 3; return i + 1; }
        if (!c.pk_offsets && !c.msg_offsets) break;                       // uniform: every item is the first
    }
    *what = 0; return 0;
}

// ---- layout of a round: the uniform layout (no offset tables) where every piece shares it -- it keeps the fast forms the pipeline picks for
// uniform layouts (the staged decompression of 48-byte keys, the eight-lane key sum on the wave engine) --, ragged tables otherwise. Keys and
// messages are decided separately.
struct mbls_stream_layout { int keys_uniform, msgs_uniform; uint32_t k, msg_len; };
MBLS_SFN void stream_layout_add(mbls_stream_layout& l, bool first_piece, const mbls_stream_call_shape& c) {
    if (first_piece) { l.keys_uniform = !c.pk_offsets; l.msgs_uniform = !c.msg_offsets; l.k = c.k; l.msg_len = c.msg_len; return; }
    if (c.pk_offsets || c.k != l.k) l.keys_uniform = 0;
    if (c.msg_offsets || c.msg_len != l.msg_len) l.msgs_uniform = 0;
}

// ---- scatter of a piece's accept bits into the caller's bitmap. The piece covers bits [call_first, call_first + items) of the call's bitmap
// and results [round_first, ...) of the round. It touches words [w0, w0 + nw); a word entirely inside the piece is stored whole, a boundary
// word (shared with the call's other pieces) is OR-ed in.
MBLS_SFN void stream_bitmap_words(uint64_t call_first, uint64_t items, uint64_t* w0, uint64_t* nw) {
    *w0 = call_first / 64; *nw = items ? (call_first + items - 1) / 64 - *w0 + 1 : 0;
}
// the bits of call word w that the piece owns (round_res: the round's result bytes); *whole = the word lies entirely inside the piece
MBLS_SFN uint64_t stream_bitmap_word(const uint8_t* round_res, uint64_t round_first, uint64_t call_first, uint64_t items, uint64_t w, int* whole) {
    const uint64_t wlo = 64 * w, lo = wlo > call_first ? wlo : call_first;
    const uint64_t hi = wlo + 64 < call_first + items ? wlo + 64 : call_first + items;
    uint64_t bits = 0;
    for (uint64_t b = lo; b < hi; b++) bits |= (uint64_t)(round_res[round_first + (b - call_first)] != 0) << (b - wlo);
    *whole = lo == wlo && hi == wlo + 64;
    return bits;
}

// ---- gather of a committee call's bitfields (k_stream_gather_cmt): a call carries fields of bits_len bytes at any address, the round's slot holds fields of
// bits_stride bytes (a multiple of 4, 4-byte aligned). Destination dword j of an item is bytes [4 j, 4 j + 4) of its field, little-endian, with every byte at or
// beyond bits_len zero: nothing outside [0, bits_len) of the field is read. `fast` (one decision per tile): the tile's first field and bits_len are both multiples
// of 4, so every field is 4-byte aligned and made of whole dwords.
MBLS_SFN int stream_bits_fast(const uint8_t* first_field, uint32_t bits_len) { return ((((uintptr_t)first_field) | bits_len) & 3u) == 0; }
MBLS_SFN uint32_t stream_bits_dword(const uint8_t* field, uint32_t bits_len, uint32_t j, int fast) {
    const uint64_t b0 = 4 * (uint64_t)j;
    if (b0 >= bits_len) return 0;
    if (fast) return *(const uint32_t*)(field + b0);
    const uint32_t left = bits_len - (uint32_t)b0, nb = left < 4 ? left : 4;
    uint32_t v = 0;
    for (uint32_t t = 0; t < nb; t++) v |= (uint32_t)field[b0 + t] << (8 * t);
    return v;
}
#endif

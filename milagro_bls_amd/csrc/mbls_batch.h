// mbls_batch.h -- one description of a per-item verification batch on its way from an entry point to a pass (mbls_fast_aggregate_verify_batch*, mbls_verify_batch*
// their _indexed and _committee forms, with per-item messages, a shared list or a resident table): where the keys come from, where the messages come from, the items and the
// outputs, and `slice`, the ONE place that knows how each pointer advances when a pass starts at item lo. Pure (no HIP call, no context): a header of its own, like
// mbls_stream.h and mbls_mtb.h, so that a host compiler can build it for the CPU tests (tests/batch_emul/mbls_batch_harness.cpp).
#ifndef MBLS_BATCH_H
#define MBLS_BATCH_H
#include <stdint.h>
#include "../../include/mbls.h"

// where an item's public keys come from
struct keysrc {
    const uint8_t* d_pks = nullptr; int fmt = MBLS_PK_UNCOMPRESSED; const uint32_t* d_off = nullptr;      // wire bytes
    const uint32_t* d_recs = nullptr; uint64_t tsize = 0; const uint32_t* d_idx = nullptr; bool indexed = false;   // key table
    const mbls_keytable* tab = nullptr;
    // committee table (mbls_cmt.h): keys of the table above (indexed, d_idx null), named per item by a committee and a bitfield
    bool committee = false; const uint32_t* d_crecs = nullptr; uint64_t ccount = 0; const uint32_t* d_members = nullptr; uint32_t cmax = 0;
    const uint32_t* d_cmt_idx = nullptr; const uint8_t* d_bits = nullptr; uint32_t bits_stride = 0; const mbls_committees* cmt = nullptr;
    // committee spans (mbls_cms.h): the committee kind with, per item, ids [d_cmt_span_off[i], d_cmt_span_off[i + 1]) of d_cmt_ids (n_cmt_ids of them) and ONE bitfield
    // over their concatenated members (d_cmt_idx null)
    bool span = false; const uint32_t* d_cmt_ids = nullptr; uint64_t n_cmt_ids = 0; const uint32_t* d_cmt_span_off = nullptr;
};
// wire keys: k per item back to back, or -- d_off -- keys [d_off[i], d_off[i + 1]) of d_pks
static inline keysrc keys_wire(const uint8_t* d_pks, int fmt, const uint32_t* d_off) {
    keysrc ks; ks.d_pks = d_pks; ks.fmt = fmt; ks.d_off = d_off; return ks;
}
// indices into the records of a key table (of `size` keys when the call was enqueued); `tab` is the handle readers order themselves against
static inline keysrc keys_table(const uint32_t* d_recs, uint64_t size, const uint32_t* d_idx, const uint32_t* d_off, const mbls_keytable* tab) {
    keysrc ks; ks.indexed = true; ks.d_recs = d_recs; ks.tsize = size; ks.d_idx = d_idx; ks.d_off = d_off; ks.tab = tab; return ks;
}
// a committee per item and a bitfield of bits_stride bytes per item over the committee records d_crecs (ccount of them when the call was enqueued, the largest of
// cmax members, their member lists in d_members); the keys are those of `keys` (keys_table with d_idx and d_off null)
static inline keysrc keys_committee(keysrc keys, const uint32_t* d_crecs, uint64_t ccount, const uint32_t* d_members, uint32_t cmax, const uint32_t* d_cmt_idx,
                                    const uint8_t* d_bits, uint32_t bits_stride, const mbls_committees* cmt) {
    keysrc ks = keys; ks.committee = true; ks.d_crecs = d_crecs; ks.ccount = ccount; ks.d_members = d_members; ks.cmax = cmax; ks.d_cmt_idx = d_cmt_idx; ks.d_bits = d_bits;
    ks.bits_stride = bits_stride; ks.cmt = cmt; return ks;
}
// a span of committees per item: keys_committee with the id of item i replaced by the ids d_cmt_ids[d_cmt_span_off[i] .. d_cmt_span_off[i + 1]) -- absolute offsets
// into an array of n_cmt_ids ids, like d_off into the keys
static inline keysrc keys_committee_span(keysrc keys, const uint32_t* d_crecs, uint64_t ccount, const uint32_t* d_members, uint32_t cmax, const uint32_t* d_cmt_ids,
                                         uint64_t n_cmt_ids, const uint32_t* d_cmt_span_off, const uint8_t* d_bits, uint32_t bits_stride, const mbls_committees* cmt) {
    keysrc ks = keys_committee(keys, d_crecs, ccount, d_members, cmax, nullptr, d_bits, bits_stride, cmt);
    ks.span = true; ks.d_cmt_ids = d_cmt_ids; ks.n_cmt_ids = n_cmt_ids; ks.d_cmt_span_off = d_cmt_span_off; return ks;
}

// where an item's message comes from: its own bytes, or index i of d_idx names one of n_msgs hashed points in a table -- the context's per-call table, which holds
// the call's list (whose bytes are then d_msgs / msg_len / d_moff), or a resident one (mbls_msgtable: n_msgs is its size when the call was enqueued)
enum { MBLS_MSGS_PER_ITEM = 0, MBLS_MSGS_LIST = 1, MBLS_MSGS_TABLE = 2 };
struct msgsrc {
    int kind = MBLS_MSGS_PER_ITEM;
    const uint8_t* d_msgs = nullptr; uint32_t msg_len = 0; const uint64_t* d_moff = nullptr;
    const uint32_t* d_idx = nullptr; uint64_t n_msgs = 0;
    const mbls_shared_msgs_plan* list = nullptr;      // non-null: the pass hashes the list itself (a one-pass plan: on its message stream, beside the other front phases)
    const uint32_t* tab = nullptr; uint64_t tstride = 0; const uint32_t* flags = nullptr;      // the table the gather reads
    bool indexed() const { return kind != MBLS_MSGS_PER_ITEM; }
};
static inline msgsrc msgs_per_item(const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff) {
    msgsrc ms; ms.d_msgs = d_msgs; ms.msg_len = msg_len; ms.d_moff = d_moff; return ms;
}
// (the table's pointers follow once the context's table is reserved for n_msgs messages)
static inline msgsrc msgs_list(const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_moff, uint64_t n_msgs, const uint32_t* d_idx) {
    msgsrc ms = msgs_per_item(d_msgs, msg_len, d_moff); ms.kind = MBLS_MSGS_LIST; ms.n_msgs = n_msgs; ms.d_idx = d_idx; return ms;
}
static inline msgsrc msgs_table(const uint32_t* tab, uint64_t tstride, const uint32_t* flags, uint64_t size, const uint32_t* d_idx) {
    msgsrc ms; ms.kind = MBLS_MSGS_TABLE; ms.tab = tab; ms.tstride = tstride; ms.flags = flags; ms.n_msgs = size; ms.d_idx = d_idx; return ms;
}

struct batch {
    const uint8_t* d_sigs = nullptr; msgsrc ms; keysrc ks;
    uint64_t n = 0; uint32_t k = 0; int mode = 0;
    uint8_t* d_results = nullptr; uint64_t* d_bitmap = nullptr; uint32_t* d_status = nullptr;
};
// Items [lo, hi) of a batch as a batch of their own: uniform layouts advance the base pointers, offset tables are absolute (their slice goes with the unmoved
// base); lo is a multiple of 64 wherever there is a bitmap, so the bitmap advances by whole words. A table of hashed points does not advance -- the indices do --,
// and a list is hashed by a whole call's only pass or before the first: never by a slice. Null stays null (the keys of a pass queued before they are uploaded,
// the bytes of empty messages).
static inline batch slice(const batch& b, uint64_t lo, uint64_t hi) {
    batch t = b;
    t.n = hi - lo;
    if (b.d_sigs) t.d_sigs = b.d_sigs + 96 * lo;
    if (b.d_results) t.d_results = b.d_results + lo;
    if (b.d_bitmap) t.d_bitmap = b.d_bitmap + lo / 64;
    if (b.d_status) t.d_status = b.d_status + lo;
    if (b.ks.committee) {        // one committee id -- a span: one range of the (unmoved) id array, its offsets absolute -- and one bitfield per item
        if (b.ks.d_cmt_idx) t.ks.d_cmt_idx = b.ks.d_cmt_idx + lo;
        if (b.ks.d_cmt_span_off) t.ks.d_cmt_span_off = b.ks.d_cmt_span_off + lo;
        if (b.ks.d_bits) t.ks.d_bits = b.ks.d_bits + (uint64_t)b.ks.bits_stride * lo;
    } else if (b.ks.d_off) t.ks.d_off = b.ks.d_off + lo;
    else {
        const uint64_t unit = b.ks.fmt == MBLS_PK_COMPRESSED ? 48 : 96;
        if (b.ks.d_pks) t.ks.d_pks = b.ks.d_pks + unit * (uint64_t)b.k * lo;
        if (b.ks.d_idx) t.ks.d_idx = b.ks.d_idx + (uint64_t)b.k * lo;
    }
    if (b.ms.indexed()) { t.ms.d_idx = b.ms.d_idx + lo; t.ms.list = nullptr; }
    else if (b.ms.d_moff) t.ms.d_moff = b.ms.d_moff + lo;
    else if (b.ms.d_msgs) t.ms.d_msgs = b.ms.d_msgs + (uint64_t)b.ms.msg_len * lo;
    return t;
}
#endif

// mbls_vmd.h -- one description of a verify_multiple call on its way from an entry point to verify_multiple_impl, vmb_impl or vbg_impl (mbls_verify_multiple*:
// one call or B batches, keys as aggregate points, wire bytes, key-table indices, committee bitfields or committee spans, messages per set, in a shared list or in
// a resident table, the shard form, locate mode): the sets, the outputs, the batches, and the two facts the second half of an _rng call passes on. It reuses the
// key and message sources of mbls_batch.h; vm_host is the same call while it is still in host memory. Pure (no HIP call, no context): a header of its own, like
// mbls_batch.h, so that a host compiler can build it for the CPU tests (tests/batch_emul/mbls_vmd_harness.cpp).
#ifndef MBLS_VMD_H
#define MBLS_VMD_H
#include "mbls_batch.h"

// A key source that names its handle alone, for entries whose checks read the table only under the context's lock and in their own order: keys_of_table /
// keys_of_committees / keys_of_committee_span then fill in what the handle holds (as msgs_in_table / msgs_of_table do for messages).
static inline keysrc keys_in_table(const mbls_keytable* t, const uint32_t* d_idx, const uint32_t* d_off) { return keys_table(nullptr, 0, d_idx, d_off, t); }
static inline keysrc keys_in_committees(const mbls_committees* t, const uint32_t* d_cmt_idx, const uint8_t* d_bits, uint32_t bits_stride) {
    return keys_committee(keys_in_table(nullptr, nullptr, nullptr), nullptr, 0, nullptr, 0, d_cmt_idx, d_bits, bits_stride, t);
}
static inline keysrc keys_in_committee_span(const mbls_committees* t, const uint32_t* d_cmt_ids, uint64_t n_cmt_ids, const uint32_t* d_cmt_span_off, const uint8_t* d_bits,
                                            uint32_t bits_stride) {
    return keys_committee_span(keys_in_table(nullptr, nullptr, nullptr), nullptr, 0, nullptr, 0, d_cmt_ids, n_cmt_ids, d_cmt_span_off, d_bits, bits_stride, t);
}

struct vm_call {
    // the sets: signatures, keys -- aggregate points (d_apks, the one kind the per-item entries do not have) or a key source with k keys per set where it has no
    // offsets --, messages (per set, or d_idx of ms naming entries of a list or of the resident table mt, of which the host has counted `named` distinct ones; 0: not
    // known), blinding scalars
    const uint8_t* d_sigs = nullptr; const uint8_t* d_apks = nullptr; keysrc ks; uint32_t k = 0;
    msgsrc ms; const mbls_msgtable* mt = nullptr; uint64_t named = 0;
    const uint64_t* d_rands = nullptr; uint64_t n = 0;
    // the outputs: one byte and one word per call (per batch where there are batches), or the shard form's record; locate mode: a byte (required) and a word per set
    uint8_t* d_result = nullptr; uint32_t* d_status_or = nullptr; uint32_t* d_partial = nullptr;
    bool locate = false; uint8_t* d_set_results = nullptr; uint32_t* d_set_status = nullptr;
    // the batches, where there are any: a table of B + 1 offsets or spb sets each; max_groups: the distinct (batch, entry) pairs where the host has counted them.
    // longest: the longest batch -- in a call without batches the longest group of sets naming one message -- where the host has counted it (0: not known)
    const uint32_t* d_boff = nullptr; uint32_t spb = 0; uint64_t B = 0, longest = 0, max_groups = 0;
    // the second half of an _rng call: k_sig has run over the signatures on this workspace and the host has seen every one pass (d_sigs is not read); the message
    // phase is already on the context's message stream
    bool sigs_resident = false, hash_enqueued = false;

    vm_call keys_apks(const uint8_t* d) const { vm_call v = *this; v.d_apks = d; v.ks = keysrc(); v.k = 0; return v; }
    vm_call keys(const keysrc& s, uint32_t per_set) const { vm_call v = *this; v.d_apks = nullptr; v.ks = s; v.k = per_set; return v; }
    vm_call msgs(const msgsrc& m) const { vm_call v = *this; v.ms = m; v.mt = nullptr; v.named = 0; return v; }
    vm_call msgs_in(const mbls_msgtable* t, const uint32_t* d_idx, uint64_t named_entries) const {
        vm_call v = *this; v.ms = msgs_table(nullptr, 0, nullptr, 0, d_idx); v.mt = t; v.named = named_entries; return v;
    }
    vm_call out(uint8_t* result, uint32_t* status_or) const { vm_call v = *this; v.d_result = result; v.d_status_or = status_or; v.d_partial = nullptr; return v; }
    vm_call out_partial(uint32_t* partial) const { vm_call v = *this; v.d_result = nullptr; v.d_status_or = nullptr; v.d_partial = partial; return v; }
    vm_call out_sets(uint8_t* set_results, uint32_t* set_status) const { vm_call v = *this; v.locate = true; v.d_set_results = set_results; v.d_set_status = set_status; return v; }
    vm_call batches(const uint32_t* boff, uint32_t sets_per_batch, uint64_t n_batches, uint64_t groups) const {
        vm_call v = *this; v.d_boff = boff; v.spb = sets_per_batch; v.B = n_batches; v.max_groups = groups; return v;
    }
    vm_call counted(uint64_t longest_range) const { vm_call v = *this; v.longest = longest_range; return v; }
    vm_call second_half(const uint64_t* rands, bool hash_on_its_stream) const {
        vm_call v = *this; v.d_sigs = nullptr; v.d_rands = rands; v.sigs_resident = true; v.hash_enqueued = hash_on_its_stream; return v;
    }
};
static inline vm_call vm_sets(const uint8_t* d_sigs, const uint64_t* d_rands, uint64_t n) { vm_call v; v.d_sigs = d_sigs; v.d_rands = d_rands; v.n = n; return v; }

// which key phase a call runs, in the order verify_multiple_impl asks: the makers leave exactly one kind standing
enum { VM_KEYS_SPAN = 0, VM_KEYS_COMMITTEE = 1, VM_KEYS_TABLE = 2, VM_KEYS_WIRE = 3, VM_KEYS_APKS = 4 };
static inline int vm_key_kind(const vm_call& v) {
    if (v.ks.span) return VM_KEYS_SPAN;
    if (v.ks.committee) return VM_KEYS_COMMITTEE;
    if (v.ks.indexed) return VM_KEYS_TABLE;
    if (!v.d_apks) return VM_KEYS_WIRE;
    return VM_KEYS_APKS;
}

// The same call in host memory (the host and _rng entries): ms holds host pointers, hc the committee or span form's ids and bitfields (apks96 is then null),
// rands the caller's scalars or draw / user the source they are drawn from.
struct host_committees;
struct vm_host {
    const uint8_t* sigs96 = nullptr; const uint8_t* apks96 = nullptr; const host_committees* hc = nullptr;
    msgsrc ms; const mbls_msgtable* mt = nullptr;
    const uint64_t* rands = nullptr; mbls_scalar_source draw = nullptr; void* user = nullptr; uint64_t n = 0;
    const uint32_t* boff = nullptr; uint32_t spb = 0; uint64_t B = 0;
    uint8_t* result = nullptr; uint32_t* status = nullptr; bool locate = false; uint8_t* set_results = nullptr; uint32_t* set_status = nullptr;

    vm_host keys_apks(const uint8_t* a) const { vm_host v = *this; v.apks96 = a; v.hc = nullptr; return v; }
    vm_host keys(const host_committees* h) const { vm_host v = *this; v.apks96 = nullptr; v.hc = h; return v; }
    vm_host msgs(const msgsrc& m) const { vm_host v = *this; v.ms = m; v.mt = nullptr; return v; }
    vm_host msgs_in(const mbls_msgtable* t, const uint32_t* msg_idx) const { vm_host v = *this; v.ms = msgs_table(nullptr, 0, nullptr, 0, msg_idx); v.mt = t; return v; }
    vm_host scalars(const uint64_t* r) const { vm_host v = *this; v.rands = r; v.draw = nullptr; v.user = nullptr; return v; }
    vm_host source(mbls_scalar_source d, void* u) const { vm_host v = *this; v.rands = nullptr; v.draw = d; v.user = u; return v; }
    vm_host batches(const uint32_t* offsets, uint32_t sets_per_batch, uint64_t n_batches) const { vm_host v = *this; v.boff = offsets; v.spb = sets_per_batch; v.B = n_batches; return v; }
    vm_host out(uint8_t* r, uint32_t* s) const { vm_host v = *this; v.result = r; v.status = s; return v; }
    vm_host out_sets(uint8_t* r, uint32_t* s) const { vm_host v = *this; v.locate = true; v.set_results = r; v.set_status = s; return v; }
};
static inline vm_host vm_host_sets(const uint8_t* sigs96, uint64_t n) { vm_host v; v.sigs96 = sigs96; v.n = n; return v; }
#endif

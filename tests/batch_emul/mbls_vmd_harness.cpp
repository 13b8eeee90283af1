// The description of a verify_multiple call on the host (milagro_bls_amd/csrc/mbls_vmd.h): tests/test_vm_call_cpu.py applies the header's makers one at a time to a
// description it holds as a flat record of integers (addresses it chose; nothing is dereferenced) and reads every field back.
#include <stdint.h>
#include "../../milagro_bls_amd/csrc/mbls_vmd.h"

extern "C" {
struct vd_flat {
    uint64_t sigs, apks, k, rands, n, result, status_or, partial, locate, set_results, set_status, boff, spb, B, longest, max_groups, sigs_resident, hash_enqueued, mt, named;
    uint64_t pks, fmt, key_off, recs, tsize, key_idx, indexed, keytab, committee, crecs, ccount, members, cmax, cmt_idx, bits, bits_stride, cmt, span, cmt_ids, n_cmt_ids, span_off;
    uint64_t msg_kind, msgs, msg_len, msg_off, msg_idx, n_msgs, list, tab, tstride, flags;
};
struct vh_flat {
    uint64_t sigs, apks, hc, mt, rands, draw, user, n, boff, spb, B, result, status, locate, set_results, set_status;
    uint64_t msg_kind, msgs, msg_len, msg_off, msg_idx, n_msgs, list, tab, tstride, flags;
};
}
template <typename T> static T* ptr(uint64_t a) { return (T*)(uintptr_t)a; }
template <typename T> static uint64_t addr(const T* p) { return (uint64_t)(uintptr_t)p; }

static msgsrc msgs_from(uint64_t kind, uint64_t msgs, uint64_t msg_len, uint64_t msg_off, uint64_t msg_idx, uint64_t n_msgs, uint64_t list, uint64_t tab, uint64_t tstride,
                        uint64_t flags) {
    msgsrc m; m.kind = (int)kind; m.d_msgs = ptr<const uint8_t>(msgs); m.msg_len = (uint32_t)msg_len; m.d_moff = ptr<const uint64_t>(msg_off);
    m.d_idx = ptr<const uint32_t>(msg_idx); m.n_msgs = n_msgs; m.list = ptr<const mbls_shared_msgs_plan>(list); m.tab = ptr<const uint32_t>(tab); m.tstride = tstride;
    m.flags = ptr<const uint32_t>(flags); return m;
}
static vm_call call_of(const vd_flat& f) {        // field by field, not through the makers
    vm_call v;
    v.d_sigs = ptr<const uint8_t>(f.sigs); v.d_apks = ptr<const uint8_t>(f.apks); v.k = (uint32_t)f.k; v.d_rands = ptr<const uint64_t>(f.rands); v.n = f.n;
    v.d_result = ptr<uint8_t>(f.result); v.d_status_or = ptr<uint32_t>(f.status_or); v.d_partial = ptr<uint32_t>(f.partial); v.locate = f.locate != 0;
    v.d_set_results = ptr<uint8_t>(f.set_results); v.d_set_status = ptr<uint32_t>(f.set_status); v.d_boff = ptr<const uint32_t>(f.boff); v.spb = (uint32_t)f.spb; v.B = f.B;
    v.longest = f.longest; v.max_groups = f.max_groups; v.sigs_resident = f.sigs_resident != 0; v.hash_enqueued = f.hash_enqueued != 0;
    v.mt = ptr<const mbls_msgtable>(f.mt); v.named = f.named;
    keysrc& s = v.ks;
    s.d_pks = ptr<const uint8_t>(f.pks); s.fmt = (int)f.fmt; s.d_off = ptr<const uint32_t>(f.key_off); s.d_recs = ptr<const uint32_t>(f.recs); s.tsize = f.tsize;
    s.d_idx = ptr<const uint32_t>(f.key_idx); s.indexed = f.indexed != 0; s.tab = ptr<const mbls_keytable>(f.keytab); s.committee = f.committee != 0;
    s.d_crecs = ptr<const uint32_t>(f.crecs); s.ccount = f.ccount; s.d_members = ptr<const uint32_t>(f.members); s.cmax = (uint32_t)f.cmax;
    s.d_cmt_idx = ptr<const uint32_t>(f.cmt_idx); s.d_bits = ptr<const uint8_t>(f.bits); s.bits_stride = (uint32_t)f.bits_stride; s.cmt = ptr<const mbls_committees>(f.cmt);
    s.span = f.span != 0; s.d_cmt_ids = ptr<const uint32_t>(f.cmt_ids); s.n_cmt_ids = f.n_cmt_ids; s.d_cmt_span_off = ptr<const uint32_t>(f.span_off);
    v.ms = msgs_from(f.msg_kind, f.msgs, f.msg_len, f.msg_off, f.msg_idx, f.n_msgs, f.list, f.tab, f.tstride, f.flags);
    return v;
}
static void read(const vm_call& v, vd_flat* f) {
    f->sigs = addr(v.d_sigs); f->apks = addr(v.d_apks); f->k = v.k; f->rands = addr(v.d_rands); f->n = v.n; f->result = addr(v.d_result); f->status_or = addr(v.d_status_or);
    f->partial = addr(v.d_partial); f->locate = v.locate; f->set_results = addr(v.d_set_results); f->set_status = addr(v.d_set_status); f->boff = addr(v.d_boff); f->spb = v.spb;
    f->B = v.B; f->longest = v.longest; f->max_groups = v.max_groups; f->sigs_resident = v.sigs_resident; f->hash_enqueued = v.hash_enqueued; f->mt = addr(v.mt); f->named = v.named;
    const keysrc& s = v.ks;
    f->pks = addr(s.d_pks); f->fmt = (uint64_t)s.fmt; f->key_off = addr(s.d_off); f->recs = addr(s.d_recs); f->tsize = s.tsize; f->key_idx = addr(s.d_idx); f->indexed = s.indexed;
    f->keytab = addr(s.tab); f->committee = s.committee; f->crecs = addr(s.d_crecs); f->ccount = s.ccount; f->members = addr(s.d_members); f->cmax = s.cmax;
    f->cmt_idx = addr(s.d_cmt_idx); f->bits = addr(s.d_bits); f->bits_stride = s.bits_stride; f->cmt = addr(s.cmt); f->span = s.span; f->cmt_ids = addr(s.d_cmt_ids);
    f->n_cmt_ids = s.n_cmt_ids; f->span_off = addr(s.d_cmt_span_off);
    f->msg_kind = (uint64_t)v.ms.kind; f->msgs = addr(v.ms.d_msgs); f->msg_len = v.ms.msg_len; f->msg_off = addr(v.ms.d_moff); f->msg_idx = addr(v.ms.d_idx);
    f->n_msgs = v.ms.n_msgs; f->list = addr(v.ms.list); f->tab = addr(v.ms.tab); f->tstride = v.ms.tstride; f->flags = addr(v.ms.flags);
}
static vm_host host_of(const vh_flat& f) {
    vm_host v;
    v.sigs96 = ptr<const uint8_t>(f.sigs); v.apks96 = ptr<const uint8_t>(f.apks); v.hc = ptr<const host_committees>(f.hc); v.mt = ptr<const mbls_msgtable>(f.mt);
    v.rands = ptr<const uint64_t>(f.rands); v.draw = (mbls_scalar_source)(uintptr_t)f.draw; v.user = ptr<void>(f.user); v.n = f.n; v.boff = ptr<const uint32_t>(f.boff);
    v.spb = (uint32_t)f.spb; v.B = f.B; v.result = ptr<uint8_t>(f.result); v.status = ptr<uint32_t>(f.status); v.locate = f.locate != 0;
    v.set_results = ptr<uint8_t>(f.set_results); v.set_status = ptr<uint32_t>(f.set_status);
    v.ms = msgs_from(f.msg_kind, f.msgs, f.msg_len, f.msg_off, f.msg_idx, f.n_msgs, f.list, f.tab, f.tstride, f.flags);
    return v;
}
static void read(const vm_host& v, vh_flat* f) {
    f->sigs = addr(v.sigs96); f->apks = addr(v.apks96); f->hc = addr(v.hc); f->mt = addr(v.mt); f->rands = addr(v.rands); f->draw = (uint64_t)(uintptr_t)v.draw;
    f->user = addr(v.user); f->n = v.n; f->boff = addr(v.boff); f->spb = v.spb; f->B = v.B; f->result = addr(v.result); f->status = addr(v.status); f->locate = v.locate;
    f->set_results = addr(v.set_results); f->set_status = addr(v.set_status);
    f->msg_kind = (uint64_t)v.ms.kind; f->msgs = addr(v.ms.d_msgs); f->msg_len = v.ms.msg_len; f->msg_off = addr(v.ms.d_moff); f->msg_idx = addr(v.ms.d_idx);
    f->n_msgs = v.ms.n_msgs; f->list = addr(v.ms.list); f->tab = addr(v.ms.tab); f->tstride = v.ms.tstride; f->flags = addr(v.ms.flags);
}
// the message source of op arguments a[0 ..]: kind, then what that kind's maker of mbls_batch.h takes
static msgsrc msgs_arg(const uint64_t* a) {
    if (a[0] == MBLS_MSGS_PER_ITEM) return msgs_per_item(ptr<const uint8_t>(a[1]), (uint32_t)a[2], ptr<const uint64_t>(a[3]));
    return msgs_list(ptr<const uint8_t>(a[1]), (uint32_t)a[2], ptr<const uint64_t>(a[3]), a[4], ptr<const uint32_t>(a[5]));
}
extern "C" {
enum { VD_KEYS_APKS, VD_KEYS_WIRE, VD_KEYS_IN_TABLE, VD_KEYS_IN_COMMITTEES, VD_KEYS_IN_SPAN, VD_MSGS, VD_MSGS_IN, VD_OUT, VD_OUT_PARTIAL, VD_OUT_SETS, VD_BATCHES, VD_COUNTED,
       VD_SECOND_HALF };
void vd_sets(uint64_t sigs, uint64_t rands, uint64_t n, vd_flat* out) { read(vm_sets(ptr<const uint8_t>(sigs), ptr<const uint64_t>(rands), n), out); }
// one maker applied to the description `in`
void vd_apply(const vd_flat* in, int op, const uint64_t* a, vd_flat* out) {
    const vm_call v = call_of(*in);
    switch (op) {
    case VD_KEYS_APKS: read(v.keys_apks(ptr<const uint8_t>(a[0])), out); break;
    case VD_KEYS_WIRE: read(v.keys(keys_wire(ptr<const uint8_t>(a[0]), (int)a[1], ptr<const uint32_t>(a[2])), (uint32_t)a[3]), out); break;
    case VD_KEYS_IN_TABLE: read(v.keys(keys_in_table(ptr<const mbls_keytable>(a[0]), ptr<const uint32_t>(a[1]), ptr<const uint32_t>(a[2])), (uint32_t)a[3]), out); break;
    case VD_KEYS_IN_COMMITTEES:
        read(v.keys(keys_in_committees(ptr<const mbls_committees>(a[0]), ptr<const uint32_t>(a[1]), ptr<const uint8_t>(a[2]), (uint32_t)a[3]), 0), out); break;
    case VD_KEYS_IN_SPAN:
        read(v.keys(keys_in_committee_span(ptr<const mbls_committees>(a[0]), ptr<const uint32_t>(a[1]), a[2], ptr<const uint32_t>(a[3]), ptr<const uint8_t>(a[4]), (uint32_t)a[5]), 0),
             out); break;
    case VD_MSGS: read(v.msgs(msgs_arg(a)), out); break;
    case VD_MSGS_IN: read(v.msgs_in(ptr<const mbls_msgtable>(a[0]), ptr<const uint32_t>(a[1]), a[2]), out); break;
    case VD_OUT: read(v.out(ptr<uint8_t>(a[0]), ptr<uint32_t>(a[1])), out); break;
    case VD_OUT_PARTIAL: read(v.out_partial(ptr<uint32_t>(a[0])), out); break;
    case VD_OUT_SETS: read(v.out_sets(ptr<uint8_t>(a[0]), ptr<uint32_t>(a[1])), out); break;
    case VD_BATCHES: read(v.batches(ptr<const uint32_t>(a[0]), (uint32_t)a[1], a[2], a[3]), out); break;
    case VD_COUNTED: read(v.counted(a[0]), out); break;
    default: read(v.second_half(ptr<const uint64_t>(a[0]), a[1] != 0), out); break;
    }
}
int vd_key_kind(const vd_flat* in) { return vm_key_kind(call_of(*in)); }

enum { VH_KEYS_APKS, VH_KEYS, VH_MSGS, VH_MSGS_IN, VH_SCALARS, VH_SOURCE, VH_BATCHES, VH_OUT, VH_OUT_SETS };
void vh_sets(uint64_t sigs, uint64_t n, vh_flat* out) { read(vm_host_sets(ptr<const uint8_t>(sigs), n), out); }
void vh_apply(const vh_flat* in, int op, const uint64_t* a, vh_flat* out) {
    const vm_host v = host_of(*in);
    switch (op) {
    case VH_KEYS_APKS: read(v.keys_apks(ptr<const uint8_t>(a[0])), out); break;
    case VH_KEYS: read(v.keys(ptr<const host_committees>(a[0])), out); break;
    case VH_MSGS: read(v.msgs(msgs_arg(a)), out); break;
    case VH_MSGS_IN: read(v.msgs_in(ptr<const mbls_msgtable>(a[0]), ptr<const uint32_t>(a[1])), out); break;
    case VH_SCALARS: read(v.scalars(ptr<const uint64_t>(a[0])), out); break;
    case VH_SOURCE: read(v.source((mbls_scalar_source)(uintptr_t)a[0], ptr<void>(a[1])), out); break;
    case VH_BATCHES: read(v.batches(ptr<const uint32_t>(a[0]), (uint32_t)a[1], a[2]), out); break;
    case VH_OUT: read(v.out(ptr<uint8_t>(a[0]), ptr<uint32_t>(a[1])), out); break;
    default: read(v.out_sets(ptr<uint8_t>(a[0]), ptr<uint32_t>(a[1])), out); break;
    }
}
}

// The batch description of the per-item verification entries on the host (milagro_bls_amd/csrc/mbls_batch.h): tests/test_batch_cpu.py builds a batch through the
// header's makers from addresses it chose (nothing is dereferenced), slices it, and reads every pointer and count back as an integer.
#include <stdint.h>
#include "../../milagro_bls_amd/csrc/mbls_batch.h"

extern "C" {
struct bt_flat {
    uint64_t sigs, results, bitmap, status, n, k, mode;
    uint64_t keys_indexed, pks, fmt, key_off, recs, tsize, key_idx, keytab;
    uint64_t msg_kind, msgs, msg_len, msg_off, msg_idx, n_msgs, list, tab, tstride, flags;
};
}
template <typename T> static T* ptr(uint64_t a) { return (T*)(uintptr_t)a; }
template <typename T> static uint64_t addr(const T* p) { return (uint64_t)(uintptr_t)p; }

static batch make(const bt_flat& f) {
    batch b;
    b.d_sigs = ptr<const uint8_t>(f.sigs); b.d_results = ptr<uint8_t>(f.results); b.d_bitmap = ptr<uint64_t>(f.bitmap); b.d_status = ptr<uint32_t>(f.status);
    b.n = f.n; b.k = (uint32_t)f.k; b.mode = (int)f.mode;
    b.ks = f.keys_indexed ? keys_table(ptr<const uint32_t>(f.recs), f.tsize, ptr<const uint32_t>(f.key_idx), ptr<const uint32_t>(f.key_off), ptr<const mbls_keytable>(f.keytab))
                          : keys_wire(ptr<const uint8_t>(f.pks), (int)f.fmt, ptr<const uint32_t>(f.key_off));
    if (f.msg_kind == MBLS_MSGS_PER_ITEM) b.ms = msgs_per_item(ptr<const uint8_t>(f.msgs), (uint32_t)f.msg_len, ptr<const uint64_t>(f.msg_off));
    else if (f.msg_kind == MBLS_MSGS_LIST) {
        b.ms = msgs_list(ptr<const uint8_t>(f.msgs), (uint32_t)f.msg_len, ptr<const uint64_t>(f.msg_off), f.n_msgs, ptr<const uint32_t>(f.msg_idx));
        b.ms.tab = ptr<const uint32_t>(f.tab); b.ms.tstride = f.tstride; b.ms.flags = ptr<const uint32_t>(f.flags);
    } else b.ms = msgs_table(ptr<const uint32_t>(f.tab), f.tstride, ptr<const uint32_t>(f.flags), f.n_msgs, ptr<const uint32_t>(f.msg_idx));
    b.ms.list = ptr<const mbls_shared_msgs_plan>(f.list);
    return b;
}
static void read(const batch& b, bt_flat* f) {
    f->sigs = addr(b.d_sigs); f->results = addr(b.d_results); f->bitmap = addr(b.d_bitmap); f->status = addr(b.d_status);
    f->n = b.n; f->k = b.k; f->mode = (uint64_t)b.mode;
    f->keys_indexed = b.ks.indexed; f->pks = addr(b.ks.d_pks); f->fmt = (uint64_t)b.ks.fmt; f->key_off = addr(b.ks.d_off); f->recs = addr(b.ks.d_recs);
    f->tsize = b.ks.tsize; f->key_idx = addr(b.ks.d_idx); f->keytab = addr(b.ks.tab);
    f->msg_kind = (uint64_t)b.ms.kind; f->msgs = addr(b.ms.d_msgs); f->msg_len = b.ms.msg_len; f->msg_off = addr(b.ms.d_moff); f->msg_idx = addr(b.ms.d_idx);
    f->n_msgs = b.ms.n_msgs; f->list = addr(b.ms.list); f->tab = addr(b.ms.tab); f->tstride = b.ms.tstride; f->flags = addr(b.ms.flags);
}
extern "C" {
// the batch as the makers built it
void bt_whole(const bt_flat* in, bt_flat* out) { read(make(*in), out); }
void bt_slice(const bt_flat* in, uint64_t lo, uint64_t hi, bt_flat* out) { read(slice(make(*in), lo, hi), out); }
void bt_slice_of_slice(const bt_flat* in, uint64_t lo, uint64_t hi, uint64_t lo2, uint64_t hi2, bt_flat* out) { read(slice(slice(make(*in), lo, hi), lo2, hi2), out); }
}

//! milagro_bls-compatible facade over the C ABI of `libmbls_hip.so` (`include/mbls.h`).
//!
//! **Source only -- never compiled or run**: the build image has no Rust toolchain. It is written against the
//! public API of sigp/milagro_bls v1.5.1 (`src/lib.rs:17-22`): every re-exported type keeps its name, its methods, their argument
//! meaning and their error behaviour; the bodies call the GPU library instead of the `amcl` crate. The same ABI is exercised end to
//! end by the Python mirror (`milagro_bls_amd/api.py`) and the C++ mirror (`include/milagro_bls.hpp`), which the GPU tests run.
//!
//! Differences a caller can observe:
//! * `point` fields hold serialized points (amcl's `ECP`/`ECP2` do not exist here): `PublicKey.point` / `AggregatePublicKey.point`
//!   are the 96-byte uncompressed form, `Signature.point` / `AggregateSignature.point` the 96-byte compressed form.
//! * `BLSCurve` (`pub use amcl::bls381 as BLSCurve`, `src/lib.rs:17`) is a passthrough of the amcl crate and is not provided.
//! * The batch entry points (`batch::*`, `KeyTable`) are additions: they are what the GPU exists for.
#![allow(clippy::missing_safety_doc)]

extern crate rand;
extern crate zeroize;

use rand::Rng;
use std::os::raw::{c_char, c_int, c_void};

/// `mbls_scalar_source` of include/mbls.h
type MblsScalarSource = unsafe extern "C" fn(user: *mut c_void, out: *mut u64, count: u64);
use std::sync::Once;
use zeroize::Zeroize;

pub const G1_BYTES: usize = 48; // reference src/lib.rs:20
pub const G2_BYTES: usize = 96;
pub const SECRET_KEY_BYTES: usize = 32;

/// The `AmclError` variants the reference uses (`amcl::errors::AmclError`, re-exported at `src/amcl_utils.rs:11`).
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum AmclError {
    AggregateEmptyPoints,
    InvalidSecretKeySize,
    InvalidSecretKeyRange,
    InvalidPoint,
    InvalidG1Size,
    InvalidG2Size,
}

// ------------------------------------------------------------------------------------------------ the C ABI (include/mbls.h)
#[repr(C)]
pub struct MblsCtx {
    _p: [u8; 0],
}
#[repr(C)]
pub struct MblsKeyTable {
    _p: [u8; 0],
}
// (the C names, as include/mbls.h spells them: tests/test_build_cpu.py compares these declarations with the header type by type)
#[allow(non_camel_case_types)]
#[repr(C)]
pub struct mbls_msgtable {
    _p: [u8; 0],
}
#[allow(non_camel_case_types)]
#[repr(C)]
pub struct mbls_committees {
    _p: [u8; 0],
}
#[allow(non_camel_case_types)]
#[repr(C)]
pub struct mbls_stream {
    _p: [u8; 0],
}
/// `mbls_stream_opts` (0 = default)
#[allow(non_camel_case_types)]
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mbls_stream_opts {
    pub round_items: u64,
    pub round_keys: u64,
    pub round_msg_bytes: u64,
    pub depth: u32,
    pub policy: u32,
}
/// include/mbls.h `mbls_limits`: the routing limits the plan functions take (`mbls_default_limits` fills them for a device's round)
#[allow(non_camel_case_types)]
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mbls_limits {
    pub round_items: u64,
    pub coop_max_items: u64,
    pub coop_hash_max_items: u64,
    pub coop_pack_min_items: u64,
    pub coop_pack_max_items: u64,
    pub coop_hash_pack_min_items: u64,
    pub split_max_items: u64,
    pub fork_max_items: u64,
    pub hash2_max_items: u64,
    pub tracks_min_rest: u64,
    pub tracks_side_max: u64,
}
extern "C" {
    fn mbls_ctx_create(out: *mut *mut MblsCtx, device_id: c_int) -> c_int;
    fn mbls_last_error(ctx: *mut MblsCtx) -> *const c_char;
    fn mbls_pk_from_bytes(ctx: *mut MblsCtx, bytes: *const u8, len: usize, pk_out: *mut u8) -> c_int;
    fn mbls_pk_from_bytes_unchecked(ctx: *mut MblsCtx, bytes: *const u8, len: usize, pk_out: *mut u8) -> c_int;
    fn mbls_pk_from_uncompressed_bytes(ctx: *mut MblsCtx, bytes: *const u8, len: usize, pk_out: *mut u8) -> c_int;
    fn mbls_pk_as_bytes(ctx: *mut MblsCtx, pk: *const u8, out: *mut u8) -> c_int;
    fn mbls_pk_key_validate(ctx: *mut MblsCtx, pk: *const u8) -> c_int;
    fn mbls_pk_from_secret_key(ctx: *mut MblsCtx, sk: *const u8, sk_len: usize, pk_out: *mut u8) -> c_int;
    fn mbls_sig_from_bytes(ctx: *mut MblsCtx, bytes: *const u8, len: usize, sig_out: *mut u8) -> c_int;
    fn mbls_sign(ctx: *mut MblsCtx, msg: *const u8, msg_len: usize, sk: *const u8, sk_len: usize, sig_out: *mut u8) -> c_int;
    fn mbls_verify(ctx: *mut MblsCtx, sig: *const u8, msg: *const u8, msg_len: usize, pk: *const u8) -> c_int;
    fn mbls_aggregate_public_keys(ctx: *mut MblsCtx, pks96: *const u8, n: usize, apk_out: *mut u8) -> c_int;
    fn mbls_aggregate_public_key_add(ctx: *mut MblsCtx, a: *const u8, b: *const u8, out: *mut u8) -> c_int;
    fn mbls_aggregate_signature_add(ctx: *mut MblsCtx, a: *const u8, b: *const u8, out: *mut u8) -> c_int;
    fn mbls_aggregate_signatures_batch(ctx: *mut MblsCtx, sigs96: *const u8, offsets: *const u32, n: u64, k: u32, out96: *mut u8, errs: *mut u8) -> c_int;
    fn mbls_fast_aggregate_verify(ctx: *mut MblsCtx, sig: *const u8, msg: *const u8, msg_len: usize, pks96: *const u8, n_pks: usize) -> c_int;
    fn mbls_fast_aggregate_verify_pre_aggregated(ctx: *mut MblsCtx, sig: *const u8, msg: *const u8, msg_len: usize, apk: *const u8) -> c_int;
    fn mbls_aggregate_verify(ctx: *mut MblsCtx, sig: *const u8, msgs: *const u8, msg_lens: *const usize, n_msgs: usize, pks96: *const u8, n_pks: usize) -> c_int;
    fn mbls_verify_multiple_aggregate_signatures(ctx: *mut MblsCtx, sigs96: *const u8, apks96: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64,
                                                 rands: *const u64, n: usize) -> c_int;
    fn mbls_verify_multiple_aggregate_signatures_rng(ctx: *mut MblsCtx, sigs96: *const u8, apks96: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64,
                                                     n: usize, draw: MblsScalarSource, user: *mut c_void) -> c_int;
    fn mbls_sig_check_batch(ctx: *mut MblsCtx, in96: *const u8, n: u64, errs: *mut u8, in_g2: *mut u8) -> c_int;
    fn mbls_verify_multiple_shared_msgs_rng(ctx: *mut MblsCtx, sigs96: *const u8, apks96: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64,
                                            n_msgs: u64, msg_idx: *const u32, n: u64, result: *mut u8, draw: MblsScalarSource, user: *mut c_void) -> c_int;
    fn mbls_verify_multiple_shared_msgs_locate_rng(ctx: *mut MblsCtx, sigs96: *const u8, apks96: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64,
                                                   n_msgs: u64, msg_idx: *const u32, n: u64, result: *mut u8, set_results: *mut u8, set_status: *mut u32,
                                                   draw: MblsScalarSource, user: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn mbls_verify_multiple_shared_msgs_locate(ctx: *mut MblsCtx, sigs96: *const u8, apks96: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64,
                                               n_msgs: u64, msg_idx: *const u32, rands: *const u64, n: u64, result: *mut u8, status: *mut u32,
                                               set_results: *mut u8, set_status: *mut u32) -> c_int;
    #[allow(dead_code)]
    fn mbls_verify_multiple_shared_msgs_locate_device(ctx: *mut MblsCtx, d_sigs96: *const u8, d_apks96: *const u8, d_msgs: *const u8, msg_len: u32,
                                                      d_msg_offsets: *const u64, n_msgs: u64, d_msg_idx: *const u32, d_rands: *const u64, n: u64,
                                                      d_result: *mut u8, d_status: *mut u32, d_set_results: *mut u8, d_set_status: *mut u32,
                                                      stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn mbls_verify_multiple_sets_indexed_shared_msgs_locate_device(ctx: *mut MblsCtx, t: *const MblsKeyTable, d_sigs96: *const u8, d_key_idx: *const u32,
                                                                   d_offsets: *const u32, k: u32, d_msgs: *const u8, msg_len: u32, d_msg_offsets: *const u64,
                                                                   n_msgs: u64, d_msg_idx: *const u32, d_rands: *const u64, n: u64, d_result: *mut u8,
                                                                   d_status: *mut u32, d_set_results: *mut u8, d_set_status: *mut u32,
                                                                   stream: *mut c_void) -> c_int;
    fn mbls_verify_multiple_batches(ctx: *mut MblsCtx, sigs96: *const u8, apks96: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64,
                                    rands: *const u64, n_sets: u64, batch_offsets: *const u32, sets_per_batch: u32, n_batches: u64, results: *mut u8,
                                    status: *mut u32) -> c_int;
    fn mbls_verify_multiple_batches_rng(ctx: *mut MblsCtx, sigs96: *const u8, apks96: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64,
                                        n_sets: u64, batch_offsets: *const u32, sets_per_batch: u32, n_batches: u64, results: *mut u8, draw: MblsScalarSource,
                                        user: *mut c_void) -> c_int;
    fn mbls_verify_multiple_batches_locate_rng(ctx: *mut MblsCtx, sigs96: *const u8, apks96: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64,
                                               n_sets: u64, batch_offsets: *const u32, sets_per_batch: u32, n_batches: u64, results: *mut u8,
                                               set_results: *mut u8, set_status: *mut u32, draw: MblsScalarSource, user: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn mbls_verify_multiple_batches_locate(ctx: *mut MblsCtx, sigs96: *const u8, apks96: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64,
                                           rands: *const u64, n_sets: u64, batch_offsets: *const u32, sets_per_batch: u32, n_batches: u64, results: *mut u8,
                                           status: *mut u32, set_results: *mut u8, set_status: *mut u32) -> c_int;
    #[allow(dead_code)]
    fn mbls_verify_multiple_batches_locate_device(ctx: *mut MblsCtx, d_sigs96: *const u8, d_apks96: *const u8, d_pks: *const u8, pk_format: c_int,
                                                  d_pk_offsets: *const u32, k: u32, d_msgs: *const u8, msg_len: u32, d_msg_offsets: *const u64, d_rands: *const u64,
                                                  n_sets: u64, d_batch_offsets: *const u32, sets_per_batch: u32, n_batches: u64, d_results: *mut u8,
                                                  d_status: *mut u32, d_set_results: *mut u8, d_set_status: *mut u32, stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn mbls_verify_multiple_batches_locate_indexed_device(ctx: *mut MblsCtx, t: *const MblsKeyTable, d_sigs96: *const u8, d_key_idx: *const u32,
                                                          d_offsets: *const u32, k: u32, d_msgs: *const u8, msg_len: u32, d_msg_offsets: *const u64,
                                                          d_rands: *const u64, n_sets: u64, d_batch_offsets: *const u32, sets_per_batch: u32, n_batches: u64,
                                                          d_results: *mut u8, d_status: *mut u32, d_set_results: *mut u8, d_set_status: *mut u32,
                                                          stream: *mut c_void) -> c_int;
    // device buffers: for callers that keep their inputs resident (not used by the types below)
    #[allow(dead_code)]
    fn mbls_verify_multiple_batches_device(ctx: *mut MblsCtx, d_sigs96: *const u8, d_apks96: *const u8, d_pks: *const u8, pk_format: c_int, d_pk_offsets: *const u32,
                                           k: u32, d_msgs: *const u8, msg_len: u32, d_msg_offsets: *const u64, d_rands: *const u64, n_sets: u64,
                                           d_batch_offsets: *const u32, sets_per_batch: u32, n_batches: u64, d_results: *mut u8, d_status: *mut u32,
                                           stream: *mut c_void) -> c_int;
    #[allow(dead_code)]
    fn mbls_verify_multiple_batches_indexed_device(ctx: *mut MblsCtx, t: *const MblsKeyTable, d_sigs96: *const u8, d_key_idx: *const u32, d_offsets: *const u32,
                                                   k: u32, d_msgs: *const u8, msg_len: u32, d_msg_offsets: *const u64, d_rands: *const u64, n_sets: u64,
                                                   d_batch_offsets: *const u32, sets_per_batch: u32, n_batches: u64, d_results: *mut u8, d_status: *mut u32,
                                                   stream: *mut c_void) -> c_int;
    fn mbls_fast_aggregate_verify_batch(ctx: *mut MblsCtx, sigs: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64, pks: *const u8, pk_format: c_int,
                                        pk_offsets: *const u32, n: u64, k: u32, results: *mut u8, status: *mut u32) -> c_int;
    fn mbls_aggregate_verify_batch(ctx: *mut MblsCtx, sigs96: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64, pks96: *const u8,
                                   pair_offsets: *const u32, k: u32, n: u64, results: *mut u8, status: *mut u32) -> c_int;
    fn mbls_verify_batch(ctx: *mut MblsCtx, sigs: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64, pks: *const u8, pk_format: c_int, n: u64,
                         results: *mut u8, status: *mut u32) -> c_int;
    fn mbls_keytable_create(ctx: *mut MblsCtx, capacity_hint: u64, out: *mut *mut MblsKeyTable) -> c_int;
    fn mbls_keytable_destroy(t: *mut MblsKeyTable);
    fn mbls_keytable_size(t: *const MblsKeyTable) -> u64;
    fn mbls_keytable_append(t: *mut MblsKeyTable, pks: *const u8, pk_format: c_int, validate: c_int, n: u64, first_index: *mut u64, errs: *mut u8) -> c_int;
    fn mbls_keytable_get(t: *mut MblsKeyTable, first_index: u64, n: u64, pks96: *mut u8, errs: *mut u8) -> c_int;
    fn mbls_fast_aggregate_verify_batch_indexed(ctx: *mut MblsCtx, t: *const MblsKeyTable, sigs: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64,
                                                key_idx: *const u32, offsets: *const u32, n: u64, k: u32, results: *mut u8, status: *mut u32) -> c_int;
    // shared message lists (include/mbls.h): n_msgs messages, one index per item; every listed message is hashed once
    fn mbls_ctx_reserve_msgs(ctx: *mut MblsCtx, max_msgs: u64) -> c_int;
    // resident message table: hash a message once, verify against it in any call or stream
    fn mbls_msgtable_create(ctx: *mut MblsCtx, capacity_hint: u64, out: *mut *mut mbls_msgtable) -> c_int;
    fn mbls_msgtable_destroy(t: *mut mbls_msgtable);
    fn mbls_msgtable_size(t: *const mbls_msgtable) -> u64;
    fn mbls_msgtable_append(t: *mut mbls_msgtable, msgs: *const u8, msg_len: u32, msg_offsets: *const u64, n: u64, first_index: *mut u64) -> c_int;
    fn mbls_msgtable_get(t: *mut mbls_msgtable, first_index: u64, n: u64, out96: *mut u8, errs: *mut u8) -> c_int;
    fn mbls_msgtable_clear(t: *mut mbls_msgtable) -> c_int;
    fn mbls_fast_aggregate_verify_batch_msgtable(ctx: *mut MblsCtx, sigs: *const u8, mt: *const mbls_msgtable, msg_idx: *const u32, pks: *const u8, pk_format: c_int,
                                                 pk_offsets: *const u32, n: u64, k: u32, results: *mut u8, status: *mut u32) -> c_int;
    fn mbls_verify_batch_msgtable(ctx: *mut MblsCtx, sigs: *const u8, mt: *const mbls_msgtable, msg_idx: *const u32, pks: *const u8, pk_format: c_int, n: u64,
                                  results: *mut u8, status: *mut u32) -> c_int;
    fn mbls_fast_aggregate_verify_batch_indexed_msgtable(ctx: *mut MblsCtx, t: *const MblsKeyTable, sigs: *const u8, mt: *const mbls_msgtable, msg_idx: *const u32,
                                                         key_idx: *const u32, offsets: *const u32, n: u64, k: u32, results: *mut u8, status: *mut u32) -> c_int;
    // committee table: ordered member lists over a key table with their cached key sums; verify by committee id and participation bits
    fn mbls_committees_create(ctx: *mut MblsCtx, keytable: *mut MblsKeyTable, capacity_hint: u64, out: *mut *mut mbls_committees) -> c_int;
    fn mbls_committees_destroy(t: *mut mbls_committees);
    fn mbls_committees_count(t: *const mbls_committees) -> u64;
    fn mbls_committees_clear(t: *mut mbls_committees) -> c_int;
    fn mbls_committees_max_members(t: *const mbls_committees) -> u32;
    fn mbls_committees_append(t: *mut mbls_committees, key_idx: *const u32, offsets: *const u32, n_committees: u64, first_id: *mut u64) -> c_int;
    fn mbls_committees_get(t: *mut mbls_committees, id: u64, sum96: *mut u8, n_members: *mut u32, eligible: *mut u32) -> c_int;
    fn mbls_ctx_set_committee_route(ctx: *mut MblsCtx, mode: c_int) -> c_int;
    fn mbls_plan_committee_route(m: u32, s: u32, eligible: c_int, mode: c_int) -> c_int;
    fn mbls_ctx_reserve_committee_items(ctx: *mut MblsCtx, max_items: u64, max_members: u32) -> c_int;
    fn mbls_fast_aggregate_verify_batch_committee(ctx: *mut MblsCtx, committees: *const mbls_committees, sigs: *const u8, msgs: *const u8, msg_len: u32,
                                                  msg_offsets: *const u64, cmt_idx: *const u32, bits: *const u8, bits_stride: u32, n: u64, results: *mut u8,
                                                  status: *mut u32) -> c_int;
    fn mbls_fast_aggregate_verify_batch_committee_msgtable(ctx: *mut MblsCtx, committees: *const mbls_committees, sigs: *const u8, mt: *const mbls_msgtable,
                                                           msg_idx: *const u32, cmt_idx: *const u32, bits: *const u8, bits_stride: u32, n: u64, results: *mut u8,
                                                           status: *mut u32) -> c_int;
    // committee spans: an item names up to 64 committees (cmt_ids[cmt_off[i] .. cmt_off[i + 1])) and carries one bitfield over their concatenated members
    fn mbls_fast_aggregate_verify_batch_committee_span(ctx: *mut MblsCtx, committees: *const mbls_committees, sigs: *const u8, msgs: *const u8, msg_len: u32,
                                                       msg_offsets: *const u64, cmt_ids: *const u32, n_cmt_ids: u64, cmt_off: *const u32, bits: *const u8,
                                                       bits_stride: u32, n: u64, results: *mut u8, status: *mut u32) -> c_int;
    fn mbls_fast_aggregate_verify_batch_committee_span_msgtable(ctx: *mut MblsCtx, committees: *const mbls_committees, sigs: *const u8, mt: *const mbls_msgtable,
                                                                msg_idx: *const u32, cmt_ids: *const u32, n_cmt_ids: u64, cmt_off: *const u32, bits: *const u8,
                                                                bits_stride: u32, n: u64, results: *mut u8, status: *mut u32) -> c_int;
    fn mbls_ctx_reserve_committee_span_items(ctx: *mut MblsCtx, max_items: u64, max_item_members: u32) -> c_int;
    fn mbls_plan_committee_span(sizes: *const u32, eligible: *const u8, q: u32, bits: *const u8, bits_bytes: u32, mode: c_int, complement_mask: *mut u64,
                                n_direct_listed: *mut u32, n_missing_listed: *mut u32) -> c_int;
    fn mbls_verify_multiple_msgtable_device(ctx: *mut MblsCtx, d_sigs96: *const u8, d_apks96: *const u8, mt: *const mbls_msgtable, d_msg_idx: *const u32, d_rands: *const u64,
                                            n: u64, d_result: *mut u8, d_status: *mut u32, stream: *mut c_void) -> c_int;
    fn mbls_verify_multiple_sets_indexed_msgtable_device(ctx: *mut MblsCtx, t: *const MblsKeyTable, d_sigs96: *const u8, d_key_idx: *const u32, d_offsets: *const u32, k: u32,
                                                         mt: *const mbls_msgtable, d_msg_idx: *const u32, d_rands: *const u64, n: u64, d_result: *mut u8, d_status: *mut u32,
                                                         stream: *mut c_void) -> c_int;
    fn mbls_verify_multiple_msgtable_rng(ctx: *mut MblsCtx, sigs96: *const u8, apks96: *const u8, mt: *const mbls_msgtable, msg_idx: *const u32, n: u64, result: *mut u8,
                                         draw: MblsScalarSource, user: *mut c_void) -> c_int;
    fn mbls_verify_multiple_msgtable_locate_device(ctx: *mut MblsCtx, d_sigs96: *const u8, d_apks96: *const u8, mt: *const mbls_msgtable, d_msg_idx: *const u32,
                                                   d_rands: *const u64, n: u64, d_result: *mut u8, d_status: *mut u32, d_set_results: *mut u8, d_set_status: *mut u32,
                                                   stream: *mut c_void) -> c_int;
    fn mbls_verify_multiple_sets_indexed_msgtable_locate_device(ctx: *mut MblsCtx, t: *const MblsKeyTable, d_sigs96: *const u8, d_key_idx: *const u32, d_offsets: *const u32,
                                                                k: u32, mt: *const mbls_msgtable, d_msg_idx: *const u32, d_rands: *const u64, n: u64, d_result: *mut u8,
                                                                d_status: *mut u32, d_set_results: *mut u8, d_set_status: *mut u32, stream: *mut c_void) -> c_int;
    fn mbls_verify_multiple_msgtable_locate_rng(ctx: *mut MblsCtx, sigs96: *const u8, apks96: *const u8, mt: *const mbls_msgtable, msg_idx: *const u32, n: u64,
                                                result: *mut u8, set_results: *mut u8, set_status: *mut u32, draw: MblsScalarSource, user: *mut c_void) -> c_int;
    // verify_multiple over committee bitfields and the resident message table: a set is a committee id with its bitfield, or MBLS_VM_SET_SINGLE_KEY | key index
    fn mbls_verify_multiple_committee_msgtable_device(ctx: *mut MblsCtx, committees: *const mbls_committees, d_sigs96: *const u8, d_cmt_idx: *const u32, d_bits: *const u8,
                                                      bits_stride: u32, mt: *const mbls_msgtable, d_msg_idx: *const u32, d_rands: *const u64, n: u64, d_result: *mut u8,
                                                      d_status: *mut u32, stream: *mut c_void) -> c_int;
    fn mbls_verify_multiple_committee_msgtable_locate_device(ctx: *mut MblsCtx, committees: *const mbls_committees, d_sigs96: *const u8, d_cmt_idx: *const u32,
                                                             d_bits: *const u8, bits_stride: u32, mt: *const mbls_msgtable, d_msg_idx: *const u32, d_rands: *const u64, n: u64,
                                                             d_result: *mut u8, d_status: *mut u32, d_set_results: *mut u8, d_set_status: *mut u32, stream: *mut c_void) -> c_int;
    fn mbls_verify_multiple_committee_msgtable_rng(ctx: *mut MblsCtx, committees: *const mbls_committees, sigs96: *const u8, cmt_idx: *const u32, bits: *const u8,
                                                   bits_stride: u32, mt: *const mbls_msgtable, msg_idx: *const u32, n: u64, result: *mut u8, draw: MblsScalarSource,
                                                   user: *mut c_void) -> c_int;
    fn mbls_verify_multiple_committee_msgtable_locate_rng(ctx: *mut MblsCtx, committees: *const mbls_committees, sigs96: *const u8, cmt_idx: *const u32, bits: *const u8,
                                                          bits_stride: u32, mt: *const mbls_msgtable, msg_idx: *const u32, n: u64, result: *mut u8, set_results: *mut u8,
                                                          set_status: *mut u32, draw: MblsScalarSource, user: *mut c_void) -> c_int;
    // verify_multiple over committee spans and the resident message table: a set is a range of committee ids with one field, or the one id MBLS_VM_SET_SINGLE_KEY | key index
    fn mbls_verify_multiple_committee_span_msgtable_device(ctx: *mut MblsCtx, committees: *const mbls_committees, d_sigs96: *const u8, d_cmt_ids: *const u32, n_cmt_ids: u64,
                                                           d_cmt_off: *const u32, d_bits: *const u8, bits_stride: u32, mt: *const mbls_msgtable, d_msg_idx: *const u32,
                                                           d_rands: *const u64, n: u64, d_result: *mut u8, d_status: *mut u32, stream: *mut c_void) -> c_int;
    fn mbls_verify_multiple_committee_span_msgtable_locate_device(ctx: *mut MblsCtx, committees: *const mbls_committees, d_sigs96: *const u8, d_cmt_ids: *const u32,
                                                                  n_cmt_ids: u64, d_cmt_off: *const u32, d_bits: *const u8, bits_stride: u32, mt: *const mbls_msgtable,
                                                                  d_msg_idx: *const u32, d_rands: *const u64, n: u64, d_result: *mut u8, d_status: *mut u32,
                                                                  d_set_results: *mut u8, d_set_status: *mut u32, stream: *mut c_void) -> c_int;
    fn mbls_verify_multiple_committee_span_msgtable_rng(ctx: *mut MblsCtx, committees: *const mbls_committees, sigs96: *const u8, cmt_ids: *const u32, n_cmt_ids: u64,
                                                        cmt_off: *const u32, bits: *const u8, bits_stride: u32, mt: *const mbls_msgtable, msg_idx: *const u32, n: u64,
                                                        result: *mut u8, draw: MblsScalarSource, user: *mut c_void) -> c_int;
    fn mbls_verify_multiple_committee_span_msgtable_locate_rng(ctx: *mut MblsCtx, committees: *const mbls_committees, sigs96: *const u8, cmt_ids: *const u32, n_cmt_ids: u64,
                                                               cmt_off: *const u32, bits: *const u8, bits_stride: u32, mt: *const mbls_msgtable, msg_idx: *const u32, n: u64,
                                                               result: *mut u8, set_results: *mut u8, set_status: *mut u32, draw: MblsScalarSource,
                                                               user: *mut c_void) -> c_int;
    // many verify_multiple batches per call over committee bitfields and the resident message table: the sets above, the batches of mbls_verify_multiple_batches*
    fn mbls_verify_multiple_batches_committee_msgtable_rng(ctx: *mut MblsCtx, committees: *const mbls_committees, sigs96: *const u8, cmt_idx: *const u32, bits: *const u8,
                                                           bits_stride: u32, mt: *const mbls_msgtable, msg_idx: *const u32, n_sets: u64, batch_offsets: *const u32,
                                                           sets_per_batch: u32, n_batches: u64, results: *mut u8, draw: MblsScalarSource, user: *mut c_void) -> c_int;
    fn mbls_verify_multiple_batches_committee_msgtable_locate_rng(ctx: *mut MblsCtx, committees: *const mbls_committees, sigs96: *const u8, cmt_idx: *const u32,
                                                                  bits: *const u8, bits_stride: u32, mt: *const mbls_msgtable, msg_idx: *const u32, n_sets: u64,
                                                                  batch_offsets: *const u32, sets_per_batch: u32, n_batches: u64, results: *mut u8, set_results: *mut u8,
                                                                  set_status: *mut u32, draw: MblsScalarSource, user: *mut c_void) -> c_int;
    // many verify_multiple batches per call over committee spans and the resident message table: the span sets, the batches of the entries above
    fn mbls_verify_multiple_batches_committee_span_msgtable_rng(ctx: *mut MblsCtx, committees: *const mbls_committees, sigs96: *const u8, cmt_ids: *const u32,
                                                                n_cmt_ids: u64, cmt_off: *const u32, bits: *const u8, bits_stride: u32, mt: *const mbls_msgtable,
                                                                msg_idx: *const u32, n_sets: u64, batch_offsets: *const u32, sets_per_batch: u32, n_batches: u64,
                                                                results: *mut u8, draw: MblsScalarSource, user: *mut c_void) -> c_int;
    fn mbls_verify_multiple_batches_committee_span_msgtable_locate_rng(ctx: *mut MblsCtx, committees: *const mbls_committees, sigs96: *const u8, cmt_ids: *const u32,
                                                                       n_cmt_ids: u64, cmt_off: *const u32, bits: *const u8, bits_stride: u32, mt: *const mbls_msgtable,
                                                                       msg_idx: *const u32, n_sets: u64, batch_offsets: *const u32, sets_per_batch: u32,
                                                                       n_batches: u64, results: *mut u8, set_results: *mut u8, set_status: *mut u32,
                                                                       draw: MblsScalarSource, user: *mut c_void) -> c_int;
    fn mbls_ctx_set_vm_span_split(ctx: *mut MblsCtx, mode: c_int) -> c_int;
    fn mbls_plan_verify_multiple_span(limits: *const mbls_limits, n: u64, table_size: u64, stride_words: u64, locate: c_int, split_mode: c_int, split: *mut u32,
                                                workspace_items: *mut u64) -> c_int;
    fn mbls_stream_create_msgtable(ctx: *mut MblsCtx, mode: c_int, pk_format: c_int, t: *const MblsKeyTable, mt: *mut mbls_msgtable, opts: *const mbls_stream_opts,
                                   out: *mut *mut mbls_stream) -> c_int;
    fn mbls_stream_submit_msgidx(s: *mut mbls_stream, sigs: *const u8, msg_idx: *const u32, pks: *const u8, key_idx: *const u32, pk_offsets: *const u32, n: u64, k: u32,
                                 results: *mut u8, status: *mut u32, ticket: *mut u64) -> c_int;
    fn mbls_stream_create_committee(ctx: *mut MblsCtx, committees: *mut mbls_committees, mt: *mut mbls_msgtable, bits_stride: u32, opts: *const mbls_stream_opts,
                                    out: *mut *mut mbls_stream) -> c_int;
    fn mbls_stream_submit_committee(s: *mut mbls_stream, sigs: *const u8, msg_idx: *const u32, cmt_idx: *const u32, bits: *const u8, bits_len: u32, n: u64,
                                    results: *mut u8, status: *mut u32, ticket: *mut u64) -> c_int;
    // a verify_multiple stream over the same two tables: a call is one batch of sets, never split
    fn mbls_stream_create_vm_committee(ctx: *mut MblsCtx, committees: *mut mbls_committees, mt: *mut mbls_msgtable, bits_stride: u32, opts: *const mbls_stream_opts,
                                       out: *mut *mut mbls_stream) -> c_int;
    fn mbls_stream_submit_vm(s: *mut mbls_stream, sigs96: *const u8, cmt_idx: *const u32, bits: *const u8, bits_len: u32, msg_idx: *const u32, rands: *const u64,
                             n_sets: u64, result: *mut u8, status: *mut u32, set_results: *mut u8, set_status: *mut u32, ticket: *mut u64) -> c_int;
    fn mbls_stream_flush(s: *mut mbls_stream) -> c_int;
    fn mbls_stream_wait(s: *mut mbls_stream, ticket: u64) -> c_int;
    fn mbls_stream_destroy(s: *mut mbls_stream);
    fn mbls_fast_aggregate_verify_batch_shared_msgs(ctx: *mut MblsCtx, sigs: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64, n_msgs: u64,
                                                    msg_idx: *const u32, pks: *const u8, pk_format: c_int, pk_offsets: *const u32, n: u64, k: u32,
                                                    results: *mut u8, status: *mut u32) -> c_int;
    fn mbls_verify_batch_shared_msgs(ctx: *mut MblsCtx, sigs: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64, n_msgs: u64, msg_idx: *const u32,
                                     pks: *const u8, pk_format: c_int, n: u64, results: *mut u8, status: *mut u32) -> c_int;
    fn mbls_fast_aggregate_verify_batch_indexed_shared_msgs(ctx: *mut MblsCtx, t: *const MblsKeyTable, sigs: *const u8, msgs: *const u8, msg_len: u32,
                                                            msg_offsets: *const u64, n_msgs: u64, msg_idx: *const u32, key_idx: *const u32, offsets: *const u32,
                                                            n: u64, k: u32, results: *mut u8, status: *mut u32) -> c_int;
    // test probes of what the secret-key entries leave in device memory (include/mbls.h): every allocation of the context by name and size, and a copy of one
    #[allow(dead_code)]
    fn mbls_ctx_residue_regions(ctx: *mut MblsCtx, names: *mut c_char, bytes: *mut u64, max_regions: u32, n_regions: *mut u32, cap: *mut u64) -> c_int;
    #[allow(dead_code)]
    fn mbls_ctx_residue_read(ctx: *mut MblsCtx, region: u32, offset: u64, bytes: u64, out: *mut u8) -> c_int;
}
#[repr(C)]
pub struct MblsMulti {
    _private: [u8; 0],
}
extern "C" {
    fn mbls_multi_create(out: *mut *mut MblsMulti, device_ids: *const c_int, n_devices: c_int) -> c_int;
    fn mbls_multi_destroy(m: *mut MblsMulti);
    fn mbls_multi_device_count(m: *const MblsMulti) -> c_int;
    fn mbls_multi_fast_aggregate_verify_batch(m: *mut MblsMulti, sigs: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64, pks: *const u8,
                                              pk_format: c_int, pk_offsets: *const u32, n: u64, k: u32, results: *mut u8, status: *mut u32) -> c_int;
    fn mbls_multi_rccl_active(m: *const MblsMulti) -> c_int;
    fn mbls_multi_fast_aggregate_verify_bitmap(m: *mut MblsMulti, sigs: *const u8, msgs: *const u8, msg_len: u32, msg_offsets: *const u64, pks: *const u8,
                                               pk_format: c_int, pk_offsets: *const u32, n: u64, k: u32, bitmap: *mut u64, status: *mut u32) -> c_int;
    fn mbls_multi_verify_multiple_aggregate_signatures(m: *mut MblsMulti, sigs96: *const u8, apks96: *const u8, msgs: *const u8, msg_len: u32,
                                                       msg_offsets: *const u64, rands: *const u64, n: usize) -> c_int;
    fn mbls_multi_verify_multiple_aggregate_signatures_rng(m: *mut MblsMulti, sigs96: *const u8, apks96: *const u8, msgs: *const u8, msg_len: u32,
                                                           msg_offsets: *const u64, n: usize, draw: MblsScalarSource, user: *mut c_void) -> c_int;
}
const PK_COMPRESSED: c_int = 0;
const PK_UNCOMPRESSED: c_int = 1;

struct CtxPtr(*mut MblsCtx);
unsafe impl Send for CtxPtr {}
unsafe impl Sync for CtxPtr {} // every ABI entry takes the context's lock (include/mbls.h)
static INIT: Once = Once::new();
static mut CTX: CtxPtr = CtxPtr(std::ptr::null_mut());

/// The process-wide context (GPU 0, or `MBLS_DEVICE`). There is no CPU fallback: without an MI355X this panics, like a missing
/// dynamic library would.
fn ctx() -> *mut MblsCtx {
    unsafe {
        INIT.call_once(|| {
            let dev = std::env::var("MBLS_DEVICE").ok().and_then(|s| s.parse().ok()).unwrap_or(0);
            let mut p: *mut MblsCtx = std::ptr::null_mut();
            let rc = mbls_ctx_create(&mut p, dev);
            if rc != 0 {
                panic!("mbls_ctx_create failed ({}): no MI355X / HIP device -- libmbls_hip has no CPU fallback", rc);
            }
            CTX = CtxPtr(p);
        });
        CTX.0
    }
}

fn err(code: c_int) -> AmclError {
    match code {
        1 => AmclError::InvalidG1Size,
        2 => AmclError::InvalidG2Size,
        3 => AmclError::InvalidPoint,
        4 => AmclError::AggregateEmptyPoints,
        5 => AmclError::InvalidSecretKeySize,
        6 => AmclError::InvalidSecretKeyRange,
        _ => {
            let msg = unsafe { std::ffi::CStr::from_ptr(mbls_last_error(ctx())) };
            panic!("mbls device error {}: {}", code, msg.to_string_lossy())
        }
    }
}
fn check(code: c_int) -> Result<(), AmclError> {
    if code == 0 {
        Ok(())
    } else {
        Err(err(code))
    }
}

// ------------------------------------------------------------------------------------------------ host-side SHA-256 / HKDF (KeyGenerate)
mod hkdf {
    const K: [u32; 64] = [
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3,
        0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
        0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
        0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
        0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
        0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2,
    ];
    pub fn sha256(msg: &[u8]) -> [u8; 32] {
        let mut h: [u32; 8] = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19];
        let mut m = msg.to_vec();
        m.push(0x80);
        while m.len() % 64 != 56 {
            m.push(0);
        }
        m.extend_from_slice(&((msg.len() as u64) * 8).to_be_bytes());
        for blk in m.chunks(64) {
            let mut w = [0u32; 64];
            for i in 0..16 {
                w[i] = u32::from_be_bytes([blk[4 * i], blk[4 * i + 1], blk[4 * i + 2], blk[4 * i + 3]]);
            }
            for i in 16..64 {
                let s0 = w[i - 15].rotate_right(7) ^ w[i - 15].rotate_right(18) ^ (w[i - 15] >> 3);
                let s1 = w[i - 2].rotate_right(17) ^ w[i - 2].rotate_right(19) ^ (w[i - 2] >> 10);
                w[i] = w[i - 16].wrapping_add(s0).wrapping_add(w[i - 7]).wrapping_add(s1);
            }
            let (mut a, mut b, mut c, mut d, mut e, mut f, mut g, mut hh) = (h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]);
            for i in 0..64 {
                let t1 = hh.wrapping_add(e.rotate_right(6) ^ e.rotate_right(11) ^ e.rotate_right(25)).wrapping_add((e & f) ^ (!e & g)).wrapping_add(K[i]).wrapping_add(w[i]);
                let t2 = (a.rotate_right(2) ^ a.rotate_right(13) ^ a.rotate_right(22)).wrapping_add((a & b) ^ (a & c) ^ (b & c));
                hh = g; g = f; f = e; e = d.wrapping_add(t1); d = c; c = b; b = a; a = t1.wrapping_add(t2);
            }
            for (x, y) in h.iter_mut().zip([a, b, c, d, e, f, g, hh].iter()) {
                *x = x.wrapping_add(*y);
            }
        }
        let mut out = [0u8; 32];
        for i in 0..8 {
            out[4 * i..4 * i + 4].copy_from_slice(&h[i].to_be_bytes());
        }
        out
    }
    pub fn hmac(key: &[u8], msg: &[u8]) -> [u8; 32] {
        let mut k = if key.len() > 64 { sha256(key).to_vec() } else { key.to_vec() };
        k.resize(64, 0);
        let mut i: Vec<u8> = k.iter().map(|b| b ^ 0x36).collect();
        i.extend_from_slice(msg);
        let mut o: Vec<u8> = k.iter().map(|b| b ^ 0x5c).collect();
        o.extend_from_slice(&sha256(&i));
        sha256(&o)
    }
    /// OS2IP(48 bytes) mod r as 32 big-endian bytes (bitwise long division; host-only, once per key).
    pub fn mod_r(okm: &[u8]) -> [u8; 32] {
        const R: [u32; 9] = [0x0000_0001, 0xffff_ffff, 0xfffe_5bfe, 0x53bd_a402, 0x09a1_d805, 0x3339_d808, 0x299d_7d48, 0x73ed_a753, 0];
        let mut a = [0u32; 9];
        for bit in 0..okm.len() * 8 {
            for j in (1..9).rev() {
                a[j] = (a[j] << 1) | (a[j - 1] >> 31);
            }
            a[0] = (a[0] << 1) | (((okm[bit >> 3] >> (7 - (bit & 7))) & 1) as u32);
            let mut ge = true;
            for j in (0..9).rev() {
                if a[j] != R[j] {
                    ge = a[j] > R[j];
                    break;
                }
            }
            if ge {
                let mut br = 0u64;
                for j in 0..9 {
                    let d = (a[j] as u64).wrapping_sub(R[j] as u64).wrapping_sub(br);
                    a[j] = d as u32;
                    br = (d >> 63) & 1;
                }
            }
        }
        let mut o = [0u8; 32];
        for j in 0..8 {
            o[4 * j..4 * j + 4].copy_from_slice(&a[7 - j].to_be_bytes());
        }
        o
    }
}

// ------------------------------------------------------------------------------------------------ keys (reference src/keys.rs)
/// Domain for key generation (`src/keys.rs:24`).
pub const KEY_SALT: &[u8] = b"BLS-SIG-KEYGEN-SALT-";
/// L = ceil((3 * ceil(log2(r))) / 16) = 48 (`src/keys.rs:26`).
pub const L: u8 = 48;
const CURVE_ORDER_BE: [u8; 32] = [
    0x73, 0xed, 0xa7, 0x53, 0x29, 0x9d, 0x7d, 0x48, 0x33, 0x39, 0xd8, 0x08, 0x09, 0xa1, 0xd8, 0x05, 0x53, 0xbd, 0xa4, 0x02, 0xff, 0xfe, 0x5b, 0xfe, 0xff, 0xff,
    0xff, 0xff, 0x00, 0x00, 0x00, 0x01,
];

/// A BLS secret key (`src/keys.rs:28-113`): 32 big-endian bytes, host-only; the scalar goes to the GPU only for signing.
#[derive(Clone)]
pub struct SecretKey {
    x: [u8; SECRET_KEY_BYTES],
}
impl SecretKey {
    /// `src/keys.rs:36-39`
    pub fn random<R: Rng + ?Sized>(rng: &mut R) -> Self {
        let ikm: [u8; 32] = rng.gen();
        Self::key_generate(&ikm, &[]).unwrap() // will only error if ikm < 32 bytes
    }
    /// KeyGenerate, `src/keys.rs:45-77`.
    pub fn key_generate(ikm: &[u8], key_info: &[u8]) -> Result<Self, AmclError> {
        if ikm.len() < 32 {
            return Err(AmclError::InvalidSecretKeySize);
        }
        let mut sk = [0u8; 32];
        let mut salt = KEY_SALT.to_vec();
        while sk.iter().all(|b| *b == 0) {
            salt = hkdf::sha256(&salt).to_vec(); // salt = H(salt)
            let mut ikm0 = ikm.to_vec();
            ikm0.push(0);
            let prk = hkdf::hmac(&salt, &ikm0); // PRK = HKDF-Extract(salt, IKM || I2OSP(0, 1))
            ikm0.zeroize();
            let mut info = key_info.to_vec();
            info.extend_from_slice(&[0, L]); // key_info || I2OSP(L, 2)
            let mut okm: Vec<u8> = Vec::with_capacity(64);
            let mut t: Vec<u8> = Vec::new();
            let mut ctr = 1u8;
            while okm.len() < L as usize {
                let mut m = t.clone();
                m.extend_from_slice(&info);
                m.push(ctr);
                ctr += 1;
                t = hkdf::hmac(&prk, &m).to_vec();
                okm.extend_from_slice(&t);
            }
            sk = hkdf::mod_r(&okm[..L as usize]); // SK = OS2IP(OKM) mod r
            okm.zeroize();
        }
        Ok(Self { x: sk })
    }
    /// `src/keys.rs:80-82`; error cases pinned by the reference tests at `src/keys.rs:285-297`.
    pub fn from_bytes(input: &[u8]) -> Result<SecretKey, AmclError> {
        if input.len() != SECRET_KEY_BYTES {
            return Err(AmclError::InvalidSecretKeySize);
        }
        if input.iter().all(|b| *b == 0) || input >= &CURVE_ORDER_BE[..] {
            return Err(AmclError::InvalidSecretKeyRange);
        }
        let mut x = [0u8; 32];
        x.copy_from_slice(input);
        Ok(Self { x })
    }
    /// `src/keys.rs:85-87`
    pub fn as_bytes(&self) -> [u8; SECRET_KEY_BYTES] {
        self.x
    }
}
impl PartialEq for SecretKey {
    fn eq(&self, other: &SecretKey) -> bool {
        self.as_bytes() == other.as_bytes()
    }
}
impl Eq for SecretKey {}
impl Drop for SecretKey {
    fn drop(&mut self) {
        self.x.zeroize(); // src/keys.rs:109-113
    }
}

/// A BLS public key (`src/keys.rs:116-187`). `point` = the 96-byte uncompressed form (x || y; infinity = 0x40 || 0..).
#[derive(Clone, PartialEq, Eq, Debug)]
pub struct PublicKey {
    pub point: [u8; 96],
}
impl PublicKey {
    /// `src/keys.rs:124-137`
    pub fn from_secret_key(sk: &SecretKey) -> Self {
        let mut p = [0u8; 96];
        let b = sk.as_bytes();
        check(unsafe { mbls_pk_from_secret_key(ctx(), b.as_ptr(), b.len(), p.as_mut_ptr()) }).expect("a SecretKey is always in range");
        PublicKey { point: p }
    }
    /// Compressed decode + KeyValidate, `src/keys.rs:140-147`.
    pub fn from_bytes(bytes: &[u8]) -> Result<PublicKey, AmclError> {
        let mut p = [0u8; 96];
        check(unsafe { mbls_pk_from_bytes(ctx(), bytes.as_ptr(), bytes.len(), p.as_mut_ptr()) })?;
        Ok(PublicKey { point: p })
    }
    /// `src/keys.rs:150-155`
    pub fn from_bytes_unchecked(bytes: &[u8]) -> Result<PublicKey, AmclError> {
        let mut p = [0u8; 96];
        check(unsafe { mbls_pk_from_bytes_unchecked(ctx(), bytes.as_ptr(), bytes.len(), p.as_mut_ptr()) })?;
        Ok(PublicKey { point: p })
    }
    /// `src/keys.rs:158-160`
    pub fn as_bytes(&self) -> [u8; G1_BYTES] {
        let mut o = [0u8; G1_BYTES];
        check(unsafe { mbls_pk_as_bytes(ctx(), self.point.as_ptr(), o.as_mut_ptr()) }).expect("a PublicKey always holds a decoded point");
        o
    }
    /// `src/keys.rs:163-165`
    pub fn as_uncompressed_bytes(&self) -> [u8; 2 * G1_BYTES] {
        self.point
    }
    /// `src/keys.rs:170-175`
    pub fn from_uncompressed_bytes(bytes: &[u8]) -> Result<PublicKey, AmclError> {
        let mut p = [0u8; 96];
        check(unsafe { mbls_pk_from_uncompressed_bytes(ctx(), bytes.as_ptr(), bytes.len(), p.as_mut_ptr()) })?;
        Ok(PublicKey { point: p })
    }
    /// KeyValidate, `src/keys.rs:181-186`.
    pub fn key_validate(&self) -> bool {
        unsafe { mbls_pk_key_validate(ctx(), self.point.as_ptr()) == 1 }
    }
}

/// `src/keys.rs:189-204`
#[derive(Clone, PartialEq, Eq)]
pub struct Keypair {
    pub sk: SecretKey,
    pub pk: PublicKey,
}
impl Keypair {
    pub fn random<R: Rng + ?Sized>(rng: &mut R) -> Self {
        let sk = SecretKey::random(rng);
        let pk = PublicKey::from_secret_key(&sk);
        Keypair { sk, pk }
    }
}

// ------------------------------------------------------------------------------------------------ signatures (reference src/signature.rs)
/// `src/signature.rs:9-51`. `point` = the 96-byte compressed form.
#[derive(Clone, PartialEq, Eq, Debug)]
pub struct Signature {
    pub point: [u8; G2_BYTES],
}
impl Signature {
    /// `src/signature.rs:17-21`
    pub fn new(msg: &[u8], sk: &SecretKey) -> Self {
        let mut s = [0u8; G2_BYTES];
        let b = sk.as_bytes();
        check(unsafe { mbls_sign(ctx(), msg.as_ptr(), msg.len(), b.as_ptr(), b.len(), s.as_mut_ptr()) }).expect("a SecretKey is always in range");
        Signature { point: s }
    }
    /// CoreVerify, `src/signature.rs:27-40`.
    pub fn verify(&self, msg: &[u8], pk: &PublicKey) -> bool {
        unsafe { mbls_verify(ctx(), self.point.as_ptr(), msg.as_ptr(), msg.len(), pk.point.as_ptr()) == 1 }
    }
    /// `src/signature.rs:43-46`
    pub fn from_bytes(bytes: &[u8]) -> Result<Signature, AmclError> {
        let mut s = [0u8; G2_BYTES];
        check(unsafe { mbls_sig_from_bytes(ctx(), bytes.as_ptr(), bytes.len(), s.as_mut_ptr()) })?;
        Ok(Signature { point: s })
    }
    /// `src/signature.rs:49-51`
    pub fn as_bytes(&self) -> [u8; G2_BYTES] {
        self.point
    }
}

// ------------------------------------------------------------------------------------------------ aggregates (reference src/aggregates.rs)
/// `src/aggregates.rs:17-78`
#[derive(Clone, PartialEq, Eq, Debug)]
pub struct AggregatePublicKey {
    pub point: [u8; 96],
}
impl AggregatePublicKey {
    /// `src/aggregates.rs:29-39`
    pub fn aggregate(public_keys: &[&PublicKey]) -> Result<Self, AmclError> {
        if public_keys.is_empty() {
            return Err(AmclError::AggregateEmptyPoints);
        }
        let flat: Vec<u8> = public_keys.iter().flat_map(|k| k.point.iter().copied()).collect();
        let mut p = [0u8; 96];
        check(unsafe { mbls_aggregate_public_keys(ctx(), flat.as_ptr(), public_keys.len(), p.as_mut_ptr()) })?;
        Ok(Self { point: p })
    }
    /// `src/aggregates.rs:46-56`
    pub fn into_aggregate(public_keys: &[PublicKey]) -> Result<Self, AmclError> {
        let refs: Vec<&PublicKey> = public_keys.iter().collect();
        Self::aggregate(&refs)
    }
    /// `src/aggregates.rs:61-63`
    pub fn from_public_key(public_key: &PublicKey) -> Self {
        Self { point: public_key.point }
    }
    /// `src/aggregates.rs:68-70`
    pub fn add(&mut self, public_key: &PublicKey) {
        let mut o = [0u8; 96];
        check(unsafe { mbls_aggregate_public_key_add(ctx(), self.point.as_ptr(), public_key.point.as_ptr(), o.as_mut_ptr()) }).expect("decoded points");
        self.point = o;
    }
    /// `src/aggregates.rs:73-77`
    pub fn add_aggregate(&mut self, aggregate_public_key: &AggregatePublicKey) {
        let mut o = [0u8; 96];
        check(unsafe { mbls_aggregate_public_key_add(ctx(), self.point.as_ptr(), aggregate_public_key.point.as_ptr(), o.as_mut_ptr()) }).expect("decoded points");
        self.point = o;
    }
}

/// `src/aggregates.rs:83-334`
#[derive(Clone, PartialEq, Eq, Debug)]
pub struct AggregateSignature {
    pub point: [u8; G2_BYTES],
}
impl Default for AggregateSignature {
    fn default() -> Self {
        Self::new()
    }
}
impl AggregateSignature {
    /// The point at infinity, `src/aggregates.rs:93-95`.
    pub fn new() -> Self {
        let mut p = [0u8; G2_BYTES];
        p[0] = 0xC0;
        Self { point: p }
    }
    /// `src/aggregates.rs:100-106` -- one batched launch (segmented G2 sum) instead of one addition per signature.
    pub fn aggregate(signatures: &[&Signature]) -> Self {
        if signatures.is_empty() {
            return Self::new();
        }
        let flat: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let mut out = [0u8; G2_BYTES];
        let mut e = 0u8;
        check(unsafe { mbls_aggregate_signatures_batch(ctx(), flat.as_ptr(), std::ptr::null(), 1, u32::try_from(signatures.len()).expect("signature counts are 32-bit"), out.as_mut_ptr(), &mut e) })
            .and_then(|_| check(e as c_int))
            .expect("Signature objects hold decodable points");
        Self { point: out }
    }
    /// `src/aggregates.rs:109-111`
    pub fn from_signature(signature: &Signature) -> Self {
        Self { point: signature.point }
    }
    /// `src/aggregates.rs:114-116`
    pub fn add(&mut self, signature: &Signature) {
        let mut o = [0u8; G2_BYTES];
        check(unsafe { mbls_aggregate_signature_add(ctx(), self.point.as_ptr(), signature.point.as_ptr(), o.as_mut_ptr()) }).expect("decodable points");
        self.point = o;
    }
    /// `src/aggregates.rs:122-124`
    pub fn add_aggregate(&mut self, aggregate_signature: &AggregateSignature) {
        let mut o = [0u8; G2_BYTES];
        check(unsafe { mbls_aggregate_signature_add(ctx(), self.point.as_ptr(), aggregate_signature.point.as_ptr(), o.as_mut_ptr()) }).expect("decodable points");
        self.point = o;
    }
    /// AggregateVerify, `src/aggregates.rs:130-170`.
    pub fn aggregate_verify(&self, msgs: &[&[u8]], public_keys: &[&PublicKey]) -> bool {
        let flat_m: Vec<u8> = msgs.iter().flat_map(|m| m.iter().copied()).collect();
        let lens: Vec<usize> = msgs.iter().map(|m| m.len()).collect();
        let flat_p: Vec<u8> = public_keys.iter().flat_map(|k| k.point.iter().copied()).collect();
        unsafe { mbls_aggregate_verify(ctx(), self.point.as_ptr(), flat_m.as_ptr(), lens.as_ptr(), msgs.len(), flat_p.as_ptr(), public_keys.len()) == 1 }
    }
    /// FastAggregateVerify, `src/aggregates.rs:177-215`.
    pub fn fast_aggregate_verify(&self, msg: &[u8], public_keys: &[&PublicKey]) -> bool {
        let flat: Vec<u8> = public_keys.iter().flat_map(|k| k.point.iter().copied()).collect();
        unsafe { mbls_fast_aggregate_verify(ctx(), self.point.as_ptr(), msg.as_ptr(), msg.len(), flat.as_ptr(), public_keys.len()) == 1 }
    }
    /// `src/aggregates.rs:223-253`
    pub fn fast_aggregate_verify_pre_aggregated(&self, msg: &[u8], aggregate_public_key: &AggregatePublicKey) -> bool {
        unsafe { mbls_fast_aggregate_verify_pre_aggregated(ctx(), self.point.as_ptr(), msg.as_ptr(), msg.len(), aggregate_public_key.point.as_ptr()) == 1 }
    }
    /// `src/aggregates.rs:261-316`. The blinding scalars are drawn from `rng` exactly as the reference does (8 random bytes,
    /// big-endian i64, absolute value, retry on zero, `:280-287`) -- and in the reference's ORDER: its loop tests set i's signature for
    /// the subgroup (`:272-275`) before it draws `rand[i]` and returns at the first signature outside G2, so a rejected batch leaves the
    /// caller's generator where the reference would. `mbls_verify_multiple_aggregate_signatures_rng` tests the signatures first and asks
    /// for the scalars of the sets before the first bad one only. (The iterator is collected first: the reference stops pulling from it
    /// at the rejected set.)
    pub fn verify_multiple_aggregate_signatures<'a, R, I>(rng: &mut R, signature_sets: I) -> bool
    where
        R: Rng + ?Sized,
        I: Iterator<Item = (&'a AggregateSignature, &'a AggregatePublicKey, &'a [u8])>,
    {
        let sets: Vec<(&AggregateSignature, &AggregatePublicKey, &[u8])> = signature_sets.collect();
        let n = sets.len();
        if n == 0 {
            return true; // e(infinity, -G1) = 1
        }
        let (mut sigs, mut apks, mut msgs) = (Vec::new(), Vec::new(), Vec::new());
        let mut moff: Vec<u64> = vec![0]; // messages of any length each (`&[u8]` per set): one buffer + an offset table
        for (s, a, m) in &sets {
            sigs.extend_from_slice(&s.point);
            apks.extend_from_slice(&a.point);
            msgs.extend_from_slice(m);
            moff.push(msgs.len() as u64);
        }
        // `draw` of mbls_verify_multiple_aggregate_signatures_rng: the scalars of the sets in front of the first bad signature, drawn as `:280-287` does
        let mut st = DrawState { rng, panic: None };
        let ok = unsafe {
            mbls_verify_multiple_aggregate_signatures_rng(ctx(), sigs.as_ptr(), apks.as_ptr(), msgs.as_ptr(), 0, moff.as_ptr(), n, draw_scalars::<R>,
                                                          &mut st as *mut DrawState<R> as *mut c_void) == 1
        };
        if let Some(payload) = st.panic.take() {
            std::panic::resume_unwind(payload);
        }
        ok
    }
    /// Not in the reference: `verify_multiple_aggregate_signatures(rng, signature_sets)` -- same sets, same bool, `rng` left in the same state --
    /// for batches whose sets share messages (`mbls_verify_multiple_shared_msgs_rng`): the messages are deduplicated here by their bytes, each
    /// distinct message is hashed once and, where it pays, the check walks one Miller loop per message instead of one per set.
    /// (Like the rest of this crate: source only, never compiled.)
    pub fn verify_multiple_aggregate_signatures_shared_msgs<'a, R, I>(rng: &mut R, signature_sets: I) -> bool
    where
        R: Rng + ?Sized,
        I: Iterator<Item = (&'a AggregateSignature, &'a AggregatePublicKey, &'a [u8])>,
    {
        Self::vm_shared(rng, signature_sets, false).0
    }
    /// The same, and in the same call (`mbls_verify_multiple_shared_msgs_locate_rng`) WHICH sets of a rejected call are the bad ones: the bool as above and
    /// one bool per set. Every set of an accepted call reads `true` (a passing batch is not examined set by set); a set of a rejected call reads what the
    /// one-set call with its scalar returns; a set at or behind the first signature outside G2 has no scalar (the reference never draws one) and reads
    /// `false`. `rng` is left where `verify_multiple_aggregate_signatures_shared_msgs` leaves it. (Like the rest of this crate: source only, never compiled.)
    pub fn verify_multiple_aggregate_signatures_shared_msgs_locate<'a, R, I>(rng: &mut R, signature_sets: I) -> (bool, Vec<bool>)
    where
        R: Rng + ?Sized,
        I: Iterator<Item = (&'a AggregateSignature, &'a AggregatePublicKey, &'a [u8])>,
    {
        Self::vm_shared(rng, signature_sets, true)
    }
    fn vm_shared<'a, R, I>(rng: &mut R, signature_sets: I, locate: bool) -> (bool, Vec<bool>)
    where
        R: Rng + ?Sized,
        I: Iterator<Item = (&'a AggregateSignature, &'a AggregatePublicKey, &'a [u8])>,
    {
        let sets: Vec<(&AggregateSignature, &AggregatePublicKey, &[u8])> = signature_sets.collect();
        let n = sets.len();
        if n == 0 {
            return (true, Vec::new());
        }
        let (mut sigs, mut apks, mut msgs) = (Vec::new(), Vec::new(), Vec::new());
        let mut moff: Vec<u64> = vec![0];
        let mut idx: Vec<u32> = Vec::with_capacity(n);
        let mut index: std::collections::HashMap<&[u8], u32> = std::collections::HashMap::new();
        for (s, a, m) in &sets {
            sigs.extend_from_slice(&s.point);
            apks.extend_from_slice(&a.point);
            let next = index.len() as u32;
            let j = *index.entry(*m).or_insert_with(|| {
                msgs.extend_from_slice(m);
                moff.push(msgs.len() as u64);
                next
            });
            idx.push(j);
        }
        let mut st = DrawState { rng, panic: None };
        let mut ok: u8 = 0;
        let mut sres: Vec<u8> = vec![0; if locate { n } else { 0 }];
        let rc = unsafe {
            if locate {
                mbls_verify_multiple_shared_msgs_locate_rng(ctx(), sigs.as_ptr(), apks.as_ptr(), msgs.as_ptr(), 0, moff.as_ptr(), index.len() as u64, idx.as_ptr(),
                                                            n as u64, &mut ok, sres.as_mut_ptr(), std::ptr::null_mut(), draw_scalars::<R>,
                                                            &mut st as *mut DrawState<R> as *mut c_void)
            } else {
                mbls_verify_multiple_shared_msgs_rng(ctx(), sigs.as_ptr(), apks.as_ptr(), msgs.as_ptr(), 0, moff.as_ptr(), index.len() as u64, idx.as_ptr(), n as u64,
                                                     &mut ok, draw_scalars::<R>, &mut st as *mut DrawState<R> as *mut c_void)
            }
        };
        if let Some(payload) = st.panic.take() {
            std::panic::resume_unwind(payload);
        }
        (rc == 0 && ok == 1, sres.iter().map(|&b| rc == 0 && b == 1).collect())
    }
    /// Not in the reference: what `verify_multiple_aggregate_signatures(rng, batch)` returns for every batch, called once per batch in order --
    /// as ONE call on the GPU (`mbls_verify_multiple_batches_rng`), for about the cost of one such call. One bool per batch; a bad batch rejects
    /// itself and nothing else. The scalars are drawn in the order those calls would draw them (for every batch, the sets in front of its first
    /// signature outside G2), so `rng` is left exactly where they would leave it.
    pub fn verify_multiple_aggregate_signatures_batches<'a, R, I, B>(rng: &mut R, batches: I) -> Result<Vec<bool>, AmclError>
    where
        R: Rng + ?Sized,
        I: Iterator<Item = B>,
        B: Iterator<Item = (&'a AggregateSignature, &'a AggregatePublicKey, &'a [u8])>,
    {
        let (mut sigs, mut apks, mut msgs) = (Vec::new(), Vec::new(), Vec::new());
        let mut moff: Vec<u64> = vec![0];
        let mut boff: Vec<u32> = vec![0];
        for b in batches {
            for (s, a, m) in b {
                sigs.extend_from_slice(&s.point);
                apks.extend_from_slice(&a.point);
                msgs.extend_from_slice(m);
                moff.push(msgs.len() as u64);
            }
            boff.push((moff.len() - 1) as u32);
        }
        let n_batches = boff.len() - 1;
        if n_batches == 0 {
            return Ok(Vec::new());
        }
        let mut res = vec![0u8; n_batches];
        let mut st = DrawState { rng, panic: None };
        let rc = unsafe {
            mbls_verify_multiple_batches_rng(ctx(), sigs.as_ptr(), apks.as_ptr(), msgs.as_ptr(), 0, moff.as_ptr(), (moff.len() - 1) as u64, boff.as_ptr(), 0,
                                             n_batches as u64, res.as_mut_ptr(), draw_scalars::<R>, &mut st as *mut DrawState<R> as *mut c_void)
        };
        if let Some(payload) = st.panic.take() {
            std::panic::resume_unwind(payload);
        }
        check(rc)?;
        Ok(res.into_iter().map(|r| r == 1).collect())
    }
    /// The same, and in the same call (`mbls_verify_multiple_batches_locate_rng`) WHICH sets of the rejected batches are the bad ones: one bool per batch as
    /// above, and per batch one bool per set. Every set of an accepted batch reads `true` -- a passing batch is not examined set by set: the batch check is
    /// the statement verify_multiple makes. A set of a rejected batch reads what the one-set batch with its scalar returns; a set at or behind the batch's
    /// first signature outside G2 has no scalar (the reference never draws one) and reads `false`. `rng` is left where
    /// `verify_multiple_aggregate_signatures_batches` leaves it.
    pub fn verify_multiple_aggregate_signatures_batches_locate<'a, R, I, B>(rng: &mut R, batches: I) -> Result<(Vec<bool>, Vec<Vec<bool>>), AmclError>
    where
        R: Rng + ?Sized,
        I: Iterator<Item = B>,
        B: Iterator<Item = (&'a AggregateSignature, &'a AggregatePublicKey, &'a [u8])>,
    {
        let (mut sigs, mut apks, mut msgs) = (Vec::new(), Vec::new(), Vec::new());
        let mut moff: Vec<u64> = vec![0];
        let mut boff: Vec<u32> = vec![0];
        for b in batches {
            for (s, a, m) in b {
                sigs.extend_from_slice(&s.point);
                apks.extend_from_slice(&a.point);
                msgs.extend_from_slice(m);
                moff.push(msgs.len() as u64);
            }
            boff.push((moff.len() - 1) as u32);
        }
        let n_batches = boff.len() - 1;
        if n_batches == 0 {
            return Ok((Vec::new(), Vec::new()));
        }
        let n_sets = moff.len() - 1;
        let mut res = vec![0u8; n_batches];
        let mut sres = vec![0u8; n_sets.max(1)];
        let mut st = DrawState { rng, panic: None };
        let rc = unsafe {
            mbls_verify_multiple_batches_locate_rng(ctx(), sigs.as_ptr(), apks.as_ptr(), msgs.as_ptr(), 0, moff.as_ptr(), n_sets as u64, boff.as_ptr(), 0,
                                                    n_batches as u64, res.as_mut_ptr(), sres.as_mut_ptr(), std::ptr::null_mut(), draw_scalars::<R>,
                                                    &mut st as *mut DrawState<R> as *mut c_void)
        };
        if let Some(payload) = st.panic.take() {
            std::panic::resume_unwind(payload);
        }
        check(rc)?;
        let per_set = (0..n_batches).map(|b| sres[boff[b] as usize..boff[b + 1] as usize].iter().map(|&r| r == 1).collect()).collect();
        Ok((res.into_iter().map(|r| r == 1).collect(), per_set))
    }
    /// `src/aggregates.rs:319-322`
    pub fn from_bytes(bytes: &[u8]) -> Result<AggregateSignature, AmclError> {
        let mut s = [0u8; G2_BYTES];
        check(unsafe { mbls_sig_from_bytes(ctx(), bytes.as_ptr(), bytes.len(), s.as_mut_ptr()) })?;
        Ok(Self { point: s })
    }
    /// `src/aggregates.rs:325-327`
    pub fn as_bytes(&self) -> [u8; G2_BYTES] {
        self.point
    }
}

// The `draw` of mbls_[multi_]verify_multiple_aggregate_signatures_rng: the scalars of the sets in front of the first bad signature, drawn as `:280-287` does.
// A panic must not unwind through the C frames of the library (the context mutex is held and GPU work is in flight): it is caught HERE, the scalars are
// zeroed so that the batch fails closed (a zero scalar is rejected), and the payload is raised again once the FFI call has returned -- what the C++ and
// Python mirrors do with an exception in their generator.
struct DrawState<'r, R: Rng + ?Sized> {
    rng: &'r mut R,
    panic: Option<Box<dyn std::any::Any + Send + 'static>>,
}
unsafe extern "C" fn draw_scalars<R: Rng + ?Sized>(user: *mut c_void, out: *mut u64, count: u64) {
    let st: &mut DrawState<R> = &mut *(user as *mut DrawState<R>);
    let out = std::slice::from_raw_parts_mut(out, count as usize);
    let r = std::panic::catch_unwind(std::panic::AssertUnwindSafe(|| {
        for o in out.iter_mut() {
            let mut rand = 0u64;
            while rand == 0 {
                let mut rand_bytes = [0u8; 8];
                st.rng.fill(&mut rand_bytes);
                rand = i64::from_be_bytes(rand_bytes).wrapping_abs() as u64;
            }
            *o = rand;
        }
    }));
    if let Err(payload) = r {
        for o in out.iter_mut() {
            *o = 0;
        }
        st.panic = Some(payload);
    }
}

// ------------------------------------------------------------------------------------------------ additions: the batch path
/// What the GPU exists for: many independent verifications per call (not part of the reference's API).
pub mod batch {
    use super::*;
    /// n x `AggregateSignature::fast_aggregate_verify`: item i = (signatures[i], messages[i], its `k` keys). One bool per item.
    pub fn fast_aggregate_verify(signatures: &[AggregateSignature], messages: &[[u8; 32]], public_keys: &[Vec<&PublicKey>]) -> Vec<bool> {
        let n = signatures.len();
        assert!(messages.len() == n && public_keys.len() == n);
        let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let msgs: Vec<u8> = messages.iter().flat_map(|m| m.iter().copied()).collect();
        let mut offsets: Vec<u32> = Vec::with_capacity(n + 1);
        let mut pks: Vec<u8> = Vec::new();
        offsets.push(0);
        for set in public_keys {
            for k in set {
                pks.extend_from_slice(&k.point);
            }
            offsets.push(u32::try_from(pks.len() / 96).expect("key indices are 32-bit"));
        }
        let mut res = vec![0u8; n];
        let rc = unsafe {
            mbls_fast_aggregate_verify_batch(ctx(), sigs.as_ptr(), msgs.as_ptr(), 32, std::ptr::null(), pks.as_ptr(), PK_UNCOMPRESSED, offsets.as_ptr(), n as u64, 0, res.as_mut_ptr(), std::ptr::null_mut())
        };
        if rc != 0 {
            err(rc);
        }
        res.into_iter().map(|b| b == 1).collect()
    }
    /// n x `AggregateSignature::aggregate_verify` (`src/aggregates.rs:130-170`): item i = (signatures[i], its messages, its keys), as many
    /// messages as keys per item (an item where they differ, or with none, is false like the reference's early return).
    pub fn aggregate_verify(signatures: &[AggregateSignature], messages: &[Vec<&[u8]>], public_keys: &[Vec<&PublicKey>]) -> Vec<bool> {
        let n = signatures.len();
        assert!(messages.len() == n && public_keys.len() == n);
        let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let mut pair_off: Vec<u32> = vec![0];
        let mut msg_off: Vec<u64> = vec![0];
        let (mut msgs, mut pks): (Vec<u8>, Vec<u8>) = (Vec::new(), Vec::new());
        let mut mismatch = vec![false; n];
        for i in 0..n {
            if messages[i].len() != public_keys[i].len() {
                mismatch[i] = true; // src/aggregates.rs:131-133: the item is false; it enters the batch without pairs
            } else {
                for (m, k) in messages[i].iter().zip(public_keys[i].iter()) {
                    msgs.extend_from_slice(m);
                    msg_off.push(msgs.len() as u64);
                    pks.extend_from_slice(&k.point);
                }
            }
            pair_off.push(u32::try_from(pks.len() / 96).expect("pair indices are 32-bit"));
        }
        let mut res = vec![0u8; n];
        let rc = unsafe {
            mbls_aggregate_verify_batch(ctx(), sigs.as_ptr(), msgs.as_ptr(), 0, msg_off.as_ptr(), pks.as_ptr(), pair_off.as_ptr(), 0, n as u64, res.as_mut_ptr(), std::ptr::null_mut())
        };
        if rc != 0 {
            err(rc);
        }
        res.into_iter().zip(mismatch).map(|(b, bad)| b == 1 && !bad).collect()
    }
    /// n x `Signature::verify`.
    pub fn verify(signatures: &[Signature], messages: &[[u8; 32]], public_keys: &[&PublicKey]) -> Vec<bool> {
        let n = signatures.len();
        assert!(messages.len() == n && public_keys.len() == n);
        let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let msgs: Vec<u8> = messages.iter().flat_map(|m| m.iter().copied()).collect();
        let pks: Vec<u8> = public_keys.iter().flat_map(|k| k.point.iter().copied()).collect();
        let mut res = vec![0u8; n];
        let rc = unsafe { mbls_verify_batch(ctx(), sigs.as_ptr(), msgs.as_ptr(), 32, std::ptr::null(), pks.as_ptr(), PK_UNCOMPRESSED, n as u64, res.as_mut_ptr(), std::ptr::null_mut()) };
        if rc != 0 {
            err(rc);
        }
        res.into_iter().map(|b| b == 1).collect()
    }
}

/// Several GPUs behind one handle (`mbls_multi_*`): items are independent (`src/aggregates.rs:177-215` keeps no state between calls), so a
/// batch is cut into contiguous shards, one per device, each staged and verified by its own host thread inside the library.
pub struct MultiGpu {
    h: *mut MblsMulti,
}
unsafe impl Send for MultiGpu {}
unsafe impl Sync for MultiGpu {}
impl MultiGpu {
    pub fn new(device_ids: &[i32]) -> Self {
        let mut h: *mut MblsMulti = std::ptr::null_mut();
        let rc = unsafe { mbls_multi_create(&mut h, device_ids.as_ptr(), device_ids.len() as c_int) };
        if rc != 0 {
            err(rc);
        }
        MultiGpu { h }
    }
    pub fn devices(&self) -> usize {
        unsafe { mbls_multi_device_count(self.h) as usize }
    }
    /// n x `AggregateSignature::fast_aggregate_verify` over all devices; messages of any length each.
    pub fn fast_aggregate_verify(&self, signatures: &[AggregateSignature], messages: &[&[u8]], public_keys: &[Vec<&PublicKey>]) -> Vec<bool> {
        let n = signatures.len();
        assert!(messages.len() == n && public_keys.len() == n);
        let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let mut msgs: Vec<u8> = Vec::new();
        let mut moff: Vec<u64> = vec![0];
        for m in messages {
            msgs.extend_from_slice(m);
            moff.push(msgs.len() as u64);
        }
        let mut offsets: Vec<u32> = vec![0];
        let mut pks: Vec<u8> = Vec::new();
        for set in public_keys {
            for k in set {
                pks.extend_from_slice(&k.point);
            }
            offsets.push(u32::try_from(pks.len() / 96).expect("key indices are 32-bit"));
        }
        let mut res = vec![0u8; n];
        let rc = unsafe {
            mbls_multi_fast_aggregate_verify_batch(self.h, sigs.as_ptr(), msgs.as_ptr(), 0, moff.as_ptr(), pks.as_ptr(), PK_UNCOMPRESSED, offsets.as_ptr(), n as u64, 0,
                                                   res.as_mut_ptr(), std::ptr::null_mut())
        };
        if rc != 0 {
            err(rc);
        }
        res.into_iter().map(|b| b == 1).collect()
    }
    /// Whether the handle's exchange steps (the accept bitmap below, `verify_multiple`'s partial records) run as RCCL all-gathers between the
    /// devices -- over xGMI on an MI355X node -- or, where RCCL could not set up a communicator, through host memory.
    pub fn rccl_active(&self) -> bool {
        unsafe { mbls_multi_rccl_active(self.h) == 1 }
    }
    /// The same verifications with the results as one packed accept bitmap (bit i % 64 of word i / 64 = item i) that every device of the
    /// handle ends up holding: each device packs its shard's bits, the words are all-gathered between the devices. Returns the words.
    pub fn fast_aggregate_verify_bitmap(&self, signatures: &[AggregateSignature], messages: &[&[u8]], public_keys: &[Vec<&PublicKey>]) -> Vec<u64> {
        let n = signatures.len();
        assert!(messages.len() == n && public_keys.len() == n);
        let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let mut msgs: Vec<u8> = Vec::new();
        let mut moff: Vec<u64> = vec![0];
        for m in messages {
            msgs.extend_from_slice(m);
            moff.push(msgs.len() as u64);
        }
        let mut offsets: Vec<u32> = vec![0];
        let mut pks: Vec<u8> = Vec::new();
        for set in public_keys {
            for k in set {
                pks.extend_from_slice(&k.point);
            }
            offsets.push(u32::try_from(pks.len() / 96).expect("key indices are 32-bit"));
        }
        let mut words = vec![0u64; (n + 63) / 64];
        let rc = unsafe {
            mbls_multi_fast_aggregate_verify_bitmap(self.h, sigs.as_ptr(), msgs.as_ptr(), 0, moff.as_ptr(), pks.as_ptr(), PK_UNCOMPRESSED, offsets.as_ptr(), n as u64, 0,
                                                    words.as_mut_ptr(), std::ptr::null_mut())
        };
        if rc != 0 {
            err(rc);
        }
        words
    }
    /// `AggregateSignature::verify_multiple_aggregate_signatures` (`src/aggregates.rs:261-316`) with the sets cut into one shard per device:
    /// every device runs its sets up to its Miller product and signature sum, the first device joins the records and finishes. Same bool.
    pub fn verify_multiple_aggregate_signatures<'a, R, I>(&self, rng: &mut R, signature_sets: I) -> bool
    where
        R: Rng + ?Sized,
        I: Iterator<Item = (&'a AggregateSignature, &'a AggregatePublicKey, &'a [u8])>,
    {
        let sets: Vec<(&AggregateSignature, &AggregatePublicKey, &[u8])> = signature_sets.collect();
        let n = sets.len();
        if n == 0 {
            return true;
        }
        let (mut sigs, mut apks, mut msgs) = (Vec::new(), Vec::new(), Vec::new());
        let mut moff: Vec<u64> = vec![0];
        for (s, a, m) in &sets {
            sigs.extend_from_slice(&s.point);
            apks.extend_from_slice(&a.point);
            msgs.extend_from_slice(m);
            moff.push(msgs.len() as u64);
        }
        // one call, the reference's RNG order (`src/aggregates.rs:272-287`): every device tests its shard's signatures first, the scalars are asked for once
        let mut st = DrawState { rng, panic: None };
        let ok = unsafe {
            mbls_multi_verify_multiple_aggregate_signatures_rng(self.h, sigs.as_ptr(), apks.as_ptr(), msgs.as_ptr(), 0, moff.as_ptr(), n, draw_scalars::<R>,
                                                                &mut st as *mut DrawState<R> as *mut c_void) == 1
        };
        if let Some(payload) = st.panic.take() {
            std::panic::resume_unwind(payload);
        }
        ok
    }
}
impl Drop for MultiGpu {
    fn drop(&mut self) {
        unsafe { mbls_multi_destroy(self.h) }
    }
}

/// Decoded public keys resident in GPU memory: decode (and KeyValidate) once, then verify by index -- the device-side analogue of
/// holding `PublicKey` objects and passing `&[&PublicKey]` (`src/aggregates.rs:177`).
pub struct KeyTable {
    h: *mut MblsKeyTable,
}
unsafe impl Send for KeyTable {}
unsafe impl Sync for KeyTable {}
impl KeyTable {
    pub fn new(capacity_hint: u64) -> Self {
        let mut h: *mut MblsKeyTable = std::ptr::null_mut();
        let rc = unsafe { mbls_keytable_create(ctx(), capacity_hint, &mut h) };
        if rc != 0 {
            err(rc);
        }
        KeyTable { h }
    }
    pub fn len(&self) -> u64 {
        unsafe { mbls_keytable_size(self.h) }
    }
    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }
    /// Appends compressed keys through `PublicKey::from_bytes` (decode + KeyValidate). Returns the index of the first new entry and
    /// one `Result` per key; a rejected key still occupies its index as an invalid entry (items naming it are rejected).
    pub fn append_compressed(&mut self, keys: &[[u8; G1_BYTES]]) -> (u64, Vec<Result<(), AmclError>>) {
        let flat: Vec<u8> = keys.iter().flat_map(|k| k.iter().copied()).collect();
        let mut first = 0u64;
        let mut errs = vec![0u8; keys.len()];
        let rc = unsafe { mbls_keytable_append(self.h, flat.as_ptr(), PK_COMPRESSED, 1, keys.len() as u64, &mut first, errs.as_mut_ptr()) };
        if rc != 0 {
            err(rc);
        }
        (first, errs.into_iter().map(|e| check(e as c_int)).collect())
    }
    /// Appends already-decoded keys (no re-validation, like `PublicKey::from_uncompressed_bytes`).
    pub fn append(&mut self, keys: &[&PublicKey]) -> u64 {
        let flat: Vec<u8> = keys.iter().flat_map(|k| k.point.iter().copied()).collect();
        let mut first = 0u64;
        let mut errs = vec![0u8; keys.len()];
        let rc = unsafe { mbls_keytable_append(self.h, flat.as_ptr(), PK_UNCOMPRESSED, 0, keys.len() as u64, &mut first, errs.as_mut_ptr()) };
        if rc != 0 {
            err(rc);
        }
        first
    }
    pub fn get(&self, index: u64) -> Result<PublicKey, AmclError> {
        let mut p = [0u8; 96];
        let mut e = 0u8;
        let rc = unsafe { mbls_keytable_get(self.h, index, 1, p.as_mut_ptr(), &mut e) };
        if rc != 0 {
            err(rc);
        }
        check(e as c_int)?;
        Ok(PublicKey { point: p })
    }
    /// n x fast_aggregate_verify with `k` table indices per item.
    pub fn fast_aggregate_verify(&self, signatures: &[AggregateSignature], messages: &[[u8; 32]], key_indices: &[u32], k: u32) -> Vec<bool> {
        let n = signatures.len();
        assert!(messages.len() == n && key_indices.len() == n * k as usize);
        let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let msgs: Vec<u8> = messages.iter().flat_map(|m| m.iter().copied()).collect();
        let mut res = vec![0u8; n];
        let rc = unsafe {
            mbls_fast_aggregate_verify_batch_indexed(ctx(), self.h, sigs.as_ptr(), msgs.as_ptr(), 32, std::ptr::null(), key_indices.as_ptr(), std::ptr::null(), n as u64, k, res.as_mut_ptr(), std::ptr::null_mut())
        };
        if rc != 0 {
            err(rc);
        }
        res.into_iter().map(|b| b == 1).collect()
    }
    /// The same over a LIST of messages: item i's message is `messages[message_indices[i]]` (the members of a committee sign the same root: every listed
    /// message is hashed to G2 once). An index that names no message of the list is a caller error (the library refuses the call).
    pub fn fast_aggregate_verify_shared_msgs(&self, signatures: &[AggregateSignature], messages: &[[u8; 32]], message_indices: &[u32], key_indices: &[u32], k: u32) -> Vec<bool> {
        let n = signatures.len();
        assert!(message_indices.len() == n && key_indices.len() == n * k as usize);
        assert!(message_indices.iter().all(|&j| (j as usize) < messages.len()));
        let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let msgs: Vec<u8> = messages.iter().flat_map(|m| m.iter().copied()).collect();
        let mut res = vec![0u8; n];
        let rc = unsafe {
            mbls_fast_aggregate_verify_batch_indexed_shared_msgs(ctx(), self.h, sigs.as_ptr(), msgs.as_ptr(), 32, std::ptr::null(), messages.len() as u64, message_indices.as_ptr(),
                                                                 key_indices.as_ptr(), std::ptr::null(), n as u64, k, res.as_mut_ptr(), std::ptr::null_mut())
        };
        if rc != 0 {
            err(rc);
        }
        res.into_iter().map(|b| b == 1).collect()
    }
}
/// Pre-allocates the context's table of hashed points for message lists of up to `max_msgs` messages (keeps allocation out of the first call).
pub fn reserve_message_list(max_msgs: u64) {
    let rc = unsafe { mbls_ctx_reserve_msgs(ctx(), max_msgs) };
    if rc != 0 {
        err(rc);
    }
}
/// n x `AggregateSignature::fast_aggregate_verify` over a list of messages, keys as decoded `PublicKey`s: item i = (signatures[i], messages[message_indices[i]], keys[i]).
pub fn fast_aggregate_verify_batch_shared_msgs(signatures: &[AggregateSignature], messages: &[&[u8]], message_indices: &[u32], keys: &[&[&PublicKey]]) -> Vec<bool> {
    let n = signatures.len();
    assert!(message_indices.len() == n && keys.len() == n);
    assert!(message_indices.iter().all(|&j| (j as usize) < messages.len()));
    let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
    let mut msgs: Vec<u8> = Vec::new();
    let mut moff: Vec<u64> = vec![0];
    for m in messages {
        msgs.extend_from_slice(m);
        moff.push(msgs.len() as u64);
    }
    let mut pks: Vec<u8> = Vec::new();
    let mut koff: Vec<u32> = vec![0];
    for ks in keys {
        for k in ks.iter() {
            pks.extend_from_slice(&k.point);
        }
        koff.push((pks.len() / 96) as u32);
    }
    let mut res = vec![0u8; n.max(1)];
    let rc = unsafe {
        mbls_fast_aggregate_verify_batch_shared_msgs(ctx(), sigs.as_ptr(), msgs.as_ptr(), 0, moff.as_ptr(), messages.len() as u64, message_indices.as_ptr(), pks.as_ptr(),
                                                     PK_UNCOMPRESSED, koff.as_ptr(), n as u64, 0, res.as_mut_ptr(), std::ptr::null_mut())
    };
    if rc != 0 {
        err(rc);
    }
    res.truncate(n);
    res.into_iter().map(|b| b == 1).collect()
}
impl Drop for KeyTable {
    fn drop(&mut self) {
        unsafe { mbls_keytable_destroy(self.h) }
    }
}

/// Hashed messages resident in GPU memory (`mbls_msgtable_*`; not part of the reference's API): every appended message is hashed to G2 once, and
/// verifications -- the functions below, `KeyTable::fast_aggregate_verify_msgtable`, or the calls of a `MessageTableStream` -- name their messages by
/// index, in any later call. Indices start at 0 and never change until `clear`. Drop the table after the streams made over it.
pub struct MessageTable {
    h: *mut mbls_msgtable,
}
unsafe impl Send for MessageTable {}
unsafe impl Sync for MessageTable {}
impl MessageTable {
    pub fn new(capacity_hint: u64) -> Self {
        let mut h: *mut mbls_msgtable = std::ptr::null_mut();
        let rc = unsafe { mbls_msgtable_create(ctx(), capacity_hint, &mut h) };
        if rc != 0 {
            err(rc);
        }
        MessageTable { h }
    }
    pub fn len(&self) -> u64 {
        unsafe { mbls_msgtable_size(self.h) }
    }
    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }
    /// Appends messages of any length each; returns the index of the first (message j is entry first + j).
    pub fn append(&mut self, messages: &[&[u8]]) -> u64 {
        let mut msgs: Vec<u8> = Vec::new();
        let mut moff: Vec<u64> = vec![0];
        for m in messages {
            msgs.extend_from_slice(m);
            moff.push(msgs.len() as u64);
        }
        let mut first = 0u64;
        let rc = unsafe { mbls_msgtable_append(self.h, msgs.as_ptr(), 0, moff.as_ptr(), messages.len() as u64, &mut first) };
        if rc != 0 {
            err(rc);
        }
        first
    }
    /// The compressed point of entry `index`: what hash_to_curve gives for its message.
    pub fn get(&self, index: u64) -> [u8; 96] {
        let mut p = [0u8; 96];
        let mut e = 0u8;
        let rc = unsafe { mbls_msgtable_get(self.h, index, 1, p.as_mut_ptr(), &mut e) };
        if rc != 0 || e != 0 {
            err(if rc != 0 { rc } else { e as c_int });
        }
        p
    }
    /// Size back to 0, capacity kept. `false`: refused, a stream made over the table has calls that have not completed.
    pub fn clear(&mut self) -> bool {
        unsafe { mbls_msgtable_clear(self.h) == 0 }
    }
    /// n x `AggregateSignature::fast_aggregate_verify`, keys as decoded `PublicKey`s: item i = (signatures[i], entry message_indices[i], keys[i]). Nothing is hashed.
    pub fn fast_aggregate_verify(&self, signatures: &[AggregateSignature], message_indices: &[u32], keys: &[&[&PublicKey]]) -> Vec<bool> {
        let n = signatures.len();
        assert!(message_indices.len() == n && keys.len() == n);
        assert!(message_indices.iter().all(|&j| (j as u64) < self.len()));
        let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let mut pks: Vec<u8> = Vec::new();
        let mut koff: Vec<u32> = vec![0];
        for ks in keys {
            for k in ks.iter() {
                pks.extend_from_slice(&k.point);
            }
            koff.push((pks.len() / 96) as u32);
        }
        let mut res = vec![0u8; n.max(1)];
        let rc = unsafe {
            mbls_fast_aggregate_verify_batch_msgtable(ctx(), sigs.as_ptr(), self.h, message_indices.as_ptr(), pks.as_ptr(), PK_UNCOMPRESSED, koff.as_ptr(), n as u64, 0,
                                                      res.as_mut_ptr(), std::ptr::null_mut())
        };
        if rc != 0 {
            err(rc);
        }
        res.truncate(n);
        res.into_iter().map(|b| b == 1).collect()
    }
    /// n x `Signature::verify`: item i = (signatures[i], entry message_indices[i], keys[i]).
    pub fn verify(&self, signatures: &[Signature], message_indices: &[u32], keys: &[&PublicKey]) -> Vec<bool> {
        let n = signatures.len();
        assert!(message_indices.len() == n && keys.len() == n);
        assert!(message_indices.iter().all(|&j| (j as u64) < self.len()));
        let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let pks: Vec<u8> = keys.iter().flat_map(|k| k.point.iter().copied()).collect();
        let mut res = vec![0u8; n.max(1)];
        let rc = unsafe {
            mbls_verify_batch_msgtable(ctx(), sigs.as_ptr(), self.h, message_indices.as_ptr(), pks.as_ptr(), PK_UNCOMPRESSED, n as u64, res.as_mut_ptr(), std::ptr::null_mut())
        };
        if rc != 0 {
            err(rc);
        }
        res.truncate(n);
        res.into_iter().map(|b| b == 1).collect()
    }
    /// `AggregateSignature::verify_multiple_aggregate_signatures` over sets (signature, aggregate key, entry index) whose messages are entries of this table
    /// (`mbls_verify_multiple_msgtable_rng`): the same bool as that function on the spelled-out messages, `rng` left in the same state, nothing hashed.
    pub fn verify_multiple_aggregate_signatures<'a, R, I>(&self, rng: &mut R, signature_sets: I) -> bool
    where
        R: Rng + ?Sized,
        I: Iterator<Item = (&'a AggregateSignature, &'a AggregatePublicKey, u32)>,
    {
        self.vm_msgtable(rng, signature_sets, false).0
    }
    /// The same, and in the same call (`mbls_verify_multiple_msgtable_locate_rng`) which sets of a rejected call are the bad ones, with the semantics of
    /// `AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs_locate`.
    pub fn verify_multiple_aggregate_signatures_locate<'a, R, I>(&self, rng: &mut R, signature_sets: I) -> (bool, Vec<bool>)
    where
        R: Rng + ?Sized,
        I: Iterator<Item = (&'a AggregateSignature, &'a AggregatePublicKey, u32)>,
    {
        self.vm_msgtable(rng, signature_sets, true)
    }
    fn vm_msgtable<'a, R, I>(&self, rng: &mut R, signature_sets: I, locate: bool) -> (bool, Vec<bool>)
    where
        R: Rng + ?Sized,
        I: Iterator<Item = (&'a AggregateSignature, &'a AggregatePublicKey, u32)>,
    {
        let sets: Vec<(&AggregateSignature, &AggregatePublicKey, u32)> = signature_sets.collect();
        let n = sets.len();
        if n == 0 {
            return (true, Vec::new());
        }
        let (mut sigs, mut apks) = (Vec::new(), Vec::new());
        let mut idx: Vec<u32> = Vec::with_capacity(n);
        for (s, a, j) in &sets {
            sigs.extend_from_slice(&s.point);
            apks.extend_from_slice(&a.point);
            idx.push(*j);
        }
        let mut st = DrawState { rng, panic: None };
        let mut ok: u8 = 0;
        let mut sres: Vec<u8> = vec![0; if locate { n } else { 0 }];
        let rc = unsafe {
            if locate {
                mbls_verify_multiple_msgtable_locate_rng(ctx(), sigs.as_ptr(), apks.as_ptr(), self.h, idx.as_ptr(), n as u64, &mut ok, sres.as_mut_ptr(), std::ptr::null_mut(),
                                                         draw_scalars::<R>, &mut st as *mut DrawState<R> as *mut c_void)
            } else {
                mbls_verify_multiple_msgtable_rng(ctx(), sigs.as_ptr(), apks.as_ptr(), self.h, idx.as_ptr(), n as u64, &mut ok, draw_scalars::<R>,
                                                  &mut st as *mut DrawState<R> as *mut c_void)
            }
        };
        if let Some(payload) = st.panic.take() {
            std::panic::resume_unwind(payload);
        }
        (rc == 0 && ok == 1, sres.iter().map(|&b| rc == 0 && b == 1).collect())
    }
}
impl Drop for MessageTable {
    fn drop(&mut self) {
        unsafe { mbls_msgtable_destroy(self.h) }
    }
}
impl KeyTable {
    /// n x fast_aggregate_verify with `k` key-table indices per item and one message-table index per item.
    pub fn fast_aggregate_verify_msgtable(&self, signatures: &[AggregateSignature], table: &MessageTable, message_indices: &[u32], key_indices: &[u32], k: u32) -> Vec<bool> {
        let n = signatures.len();
        assert!(message_indices.len() == n && key_indices.len() == n * k as usize);
        assert!(message_indices.iter().all(|&j| (j as u64) < table.len()));
        let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let mut res = vec![0u8; n.max(1)];
        let rc = unsafe {
            mbls_fast_aggregate_verify_batch_indexed_msgtable(ctx(), self.h, sigs.as_ptr(), table.h, message_indices.as_ptr(), key_indices.as_ptr(), std::ptr::null(), n as u64, k,
                                                              res.as_mut_ptr(), std::ptr::null_mut())
        };
        if rc != 0 {
            err(rc);
        }
        res.truncate(n);
        res.into_iter().map(|b| b == 1).collect()
    }
}
/// A verification stream over a `MessageTable` (`mbls_stream_create_msgtable`): calls of any size are packed into full-round launches, and a call names its
/// messages by table index. `verify` submits one call and waits for it; calls from several threads share the rounds. Drop the stream before its table.
pub struct MessageTableStream {
    h: *mut mbls_stream,
}
unsafe impl Send for MessageTableStream {}
unsafe impl Sync for MessageTableStream {}
impl MessageTableStream {
    pub fn new(table: &mut MessageTable, opts: mbls_stream_opts) -> Self {
        let mut h: *mut mbls_stream = std::ptr::null_mut();
        let rc = unsafe { mbls_stream_create_msgtable(ctx(), 0, PK_UNCOMPRESSED, std::ptr::null(), table.h, &opts, &mut h) };
        if rc != 0 {
            err(rc);
        }
        MessageTableStream { h }
    }
    /// n x fast_aggregate_verify: item i = (signatures[i], entry message_indices[i], keys[i]); an index the table does not hold when the call's round
    /// launches rejects its item.
    pub fn verify(&self, signatures: &[AggregateSignature], message_indices: &[u32], keys: &[&[&PublicKey]]) -> Vec<bool> {
        let n = signatures.len();
        assert!(n > 0 && message_indices.len() == n && keys.len() == n);
        let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let mut pks: Vec<u8> = Vec::new();
        let mut koff: Vec<u32> = vec![0];
        for ks in keys {
            for k in ks.iter() {
                pks.extend_from_slice(&k.point);
            }
            koff.push((pks.len() / 96) as u32);
        }
        let mut res = vec![0u8; n];
        let mut ticket = 0u64;
        let mut rc = unsafe {
            mbls_stream_submit_msgidx(self.h, sigs.as_ptr(), message_indices.as_ptr(), pks.as_ptr(), std::ptr::null(), koff.as_ptr(), n as u64, 0, res.as_mut_ptr(),
                                      std::ptr::null_mut(), &mut ticket)
        };
        if rc == 0 {
            rc = unsafe { mbls_stream_wait(self.h, ticket) };       // the buffers above stay valid until the call completes
        }
        if rc != 0 {
            err(rc);
        }
        res.into_iter().map(|b| b == 1).collect()
    }
    pub fn flush(&self) {
        unsafe { mbls_stream_flush(self.h) };
    }
}
/// Committees resident in GPU memory (`mbls_committees_*`; not part of the reference's API): ordered member lists of `KeyTable` indices, each kept with its full
/// key sum -- what the beacon state stores as a sync committee's `aggregate_pubkey`. A verification names a committee and carries the participation bits as SSZ
/// serializes them (bit j = member j; bits at or above the committee's size are ignored; checking a Bitlist's length stays with the caller); on the device the
/// aggregate key is the sum of the signers or, where most signed, the cached sum minus the absentees. Same bools as `KeyTable::fast_aggregate_verify_msgtable` with
/// the signers spelled out. Drop it before the key table it was made over. (Like the rest of this crate: source only, never compiled.)
pub struct CommitteeTable {
    h: *mut mbls_committees,
}
unsafe impl Send for CommitteeTable {}
unsafe impl Sync for CommitteeTable {}
impl CommitteeTable {
    pub fn new(keys: &KeyTable, capacity_hint: u64) -> Self {
        let mut h: *mut mbls_committees = std::ptr::null_mut();
        let rc = unsafe { mbls_committees_create(ctx(), keys.h, capacity_hint, &mut h) };
        if rc != 0 {
            err(rc);
        }
        CommitteeTable { h }
    }
    pub fn len(&self) -> u64 {
        unsafe { mbls_committees_count(self.h) }
    }
    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }
    /// One committee per member list (key-table indices, in member order); returns the id of the first.
    pub fn append(&mut self, committees: &[&[u32]]) -> u64 {
        let mut flat: Vec<u32> = Vec::new();
        let mut off: Vec<u32> = vec![0];
        for c in committees {
            flat.extend_from_slice(c);
            off.push(flat.len() as u32);
        }
        let mut first = 0u64;
        let rc = unsafe { mbls_committees_append(self.h, flat.as_ptr(), off.as_ptr(), committees.len() as u64, &mut first) };
        if rc != 0 {
            err(rc);
        }
        first
    }
    /// The committee's full key sum as 96 uncompressed bytes, its member count, and whether every member is a valid, finite key.
    pub fn aggregate_pubkey(&self, id: u64) -> ([u8; 96], u32, bool) {
        let mut p = [0u8; 96];
        let (mut m, mut e) = (0u32, 0u32);
        let rc = unsafe { mbls_committees_get(self.h, id, p.as_mut_ptr(), &mut m, &mut e) };
        if rc != 0 {
            err(rc);
        }
        (p, m, e != 0)
    }
    /// Count back to 0 (waits for everything enqueued over the table); the next append starts at id 0.
    pub fn clear(&mut self) -> bool {
        unsafe { mbls_committees_clear(self.h) == 0 }
    }
    /// 0: the cheaper route per item, 1: always sum the signers, 2: cached sum minus the absentees wherever the committee allows it.
    pub fn set_route(mode: i32) -> bool {
        unsafe { mbls_ctx_set_committee_route(ctx(), mode as c_int) == 0 }
    }
    /// Reserves the per-call scratch for batches of `max_items` items over committees of up to `max_members` members.
    pub fn reserve(max_items: u64, max_members: u32) -> bool {
        unsafe { mbls_ctx_reserve_committee_items(ctx(), max_items, max_members) == 0 }
    }
    /// `true`: an item with `s` of `m` members selected takes the complement route under `mode` (pure: no GPU).
    pub fn plan_route(m: u32, s: u32, eligible: bool, mode: i32) -> bool {
        unsafe { mbls_plan_committee_route(m, s, eligible as c_int, mode as c_int) == 1 }
    }
    /// Every bitfield at one stride: the bytes that cover the table's largest committee, rounded up to 4 (bytes of a field beyond that hold only bits at or
    /// above every committee's size, which the entries ignore).
    fn flatten_bits(&self, bits: &[&[u8]]) -> (Vec<u8>, u32) {
        let largest = unsafe { mbls_committees_max_members(self.h) } as usize;
        let stride = (((largest + 7) / 8).max(1) + 3) / 4 * 4;
        let mut flat = vec![0u8; stride * bits.len().max(1)];
        for (i, b) in bits.iter().enumerate() {
            let n = b.len().min(stride);
            flat[stride * i..stride * i + n].copy_from_slice(&b[..n]);
        }
        (flat, stride as u32)
    }
    /// n x `AggregateSignature::fast_aggregate_verify`: item i = (signatures[i], messages[i], the members of committee committee_ids[i] whose bit is set in bits[i]).
    pub fn fast_aggregate_verify(&self, signatures: &[AggregateSignature], messages: &[&[u8]], committee_ids: &[u32], bits: &[&[u8]]) -> Vec<bool> {
        let n = signatures.len();
        assert!(messages.len() == n && committee_ids.len() == n && bits.len() == n);
        let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let mut msgs: Vec<u8> = Vec::new();
        let mut moff: Vec<u64> = vec![0];
        for m in messages {
            msgs.extend_from_slice(m);
            moff.push(msgs.len() as u64);
        }
        let (flat, stride) = self.flatten_bits(bits);
        let mut res = vec![0u8; n.max(1)];
        let rc = unsafe {
            mbls_fast_aggregate_verify_batch_committee(ctx(), self.h, sigs.as_ptr(), msgs.as_ptr(), 0, moff.as_ptr(), committee_ids.as_ptr(), flat.as_ptr(), stride, n as u64,
                                                       res.as_mut_ptr(), std::ptr::null_mut())
        };
        if rc != 0 {
            err(rc);
        }
        res.truncate(n);
        res.into_iter().map(|b| b == 1).collect()
    }
    /// The same with the messages named by index into a `MessageTable`.
    pub fn fast_aggregate_verify_msgtable(&self, signatures: &[AggregateSignature], table: &MessageTable, message_indices: &[u32], committee_ids: &[u32],
                                          bits: &[&[u8]]) -> Vec<bool> {
        let n = signatures.len();
        assert!(message_indices.len() == n && committee_ids.len() == n && bits.len() == n);
        let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let (flat, stride) = self.flatten_bits(bits);
        let mut res = vec![0u8; n.max(1)];
        let rc = unsafe {
            mbls_fast_aggregate_verify_batch_committee_msgtable(ctx(), self.h, sigs.as_ptr(), table.h, message_indices.as_ptr(), committee_ids.as_ptr(), flat.as_ptr(), stride,
                                                                n as u64, res.as_mut_ptr(), std::ptr::null_mut())
        };
        if rc != 0 {
            err(rc);
        }
        res.truncate(n);
        res.into_iter().map(|b| b == 1).collect()
    }
    /// The ids of every item back to back with their absolute offsets, and every field at one stride: the widest field, rounded up to 4.
    fn flatten_spans(committee_ids: &[&[u32]], bits: &[&[u8]]) -> (Vec<u32>, u64, Vec<u32>, Vec<u8>, u32) {
        let mut ids: Vec<u32> = Vec::new();
        let mut off: Vec<u32> = vec![0];
        for l in committee_ids {
            ids.extend_from_slice(l);
            off.push(ids.len() as u32);
        }
        let n_ids = ids.len() as u64;
        if ids.is_empty() {
            ids.push(0);
        }
        let stride = (bits.iter().map(|b| b.len()).max().unwrap_or(0).max(1) + 3) / 4 * 4;
        let mut flat = vec![0u8; stride * bits.len().max(1)];
        for (i, b) in bits.iter().enumerate() {
            flat[stride * i..stride * i + b.len()].copy_from_slice(b);
        }
        (ids, n_ids, off, flat, stride as u32)
    }
    /// n x `AggregateSignature::fast_aggregate_verify` over attestations that span several committees (`mbls_fast_aggregate_verify_batch_committee_span`): item i =
    /// (signatures[i], messages[i], the committees committee_ids[i] in order -- at most `SPAN_MAX_COMMITTEES` --, bits[i]: ONE bitfield over their concatenated
    /// members, an Electra attestation's aggregation_bits as SSZ serializes them). A malformed item (an id that names nothing, too many ids, a field shorter than
    /// the committees' members) refuses the whole call.
    pub fn fast_aggregate_verify_spans(&self, signatures: &[AggregateSignature], messages: &[&[u8]], committee_ids: &[&[u32]], bits: &[&[u8]]) -> Vec<bool> {
        let n = signatures.len();
        assert!(messages.len() == n && committee_ids.len() == n && bits.len() == n);
        let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let mut msgs: Vec<u8> = Vec::new();
        let mut moff: Vec<u64> = vec![0];
        for m in messages {
            msgs.extend_from_slice(m);
            moff.push(msgs.len() as u64);
        }
        let (ids, n_ids, off, flat, stride) = Self::flatten_spans(committee_ids, bits);
        let mut res = vec![0u8; n.max(1)];
        let rc = unsafe {
            mbls_fast_aggregate_verify_batch_committee_span(ctx(), self.h, sigs.as_ptr(), msgs.as_ptr(), 0, moff.as_ptr(), ids.as_ptr(), n_ids, off.as_ptr(), flat.as_ptr(),
                                                            stride, n as u64, res.as_mut_ptr(), std::ptr::null_mut())
        };
        if rc != 0 {
            err(rc);
        }
        res.truncate(n);
        res.into_iter().map(|b| b == 1).collect()
    }
    /// The same with the messages named by index into a `MessageTable`.
    pub fn fast_aggregate_verify_spans_msgtable(&self, signatures: &[AggregateSignature], table: &MessageTable, message_indices: &[u32], committee_ids: &[&[u32]],
                                                bits: &[&[u8]]) -> Vec<bool> {
        let n = signatures.len();
        assert!(message_indices.len() == n && committee_ids.len() == n && bits.len() == n);
        let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let (ids, n_ids, off, flat, stride) = Self::flatten_spans(committee_ids, bits);
        let mut res = vec![0u8; n.max(1)];
        let rc = unsafe {
            mbls_fast_aggregate_verify_batch_committee_span_msgtable(ctx(), self.h, sigs.as_ptr(), table.h, message_indices.as_ptr(), ids.as_ptr(), n_ids, off.as_ptr(),
                                                                     flat.as_ptr(), stride, n as u64, res.as_mut_ptr(), std::ptr::null_mut())
        };
        if rc != 0 {
            err(rc);
        }
        res.truncate(n);
        res.into_iter().map(|b| b == 1).collect()
    }
    /// Reserves the span entries' scratch for batches of `max_items` items whose list regions take `max_item_members` words each.
    pub fn reserve_spans(max_items: u64, max_item_members: u32) -> bool {
        unsafe { mbls_ctx_reserve_committee_span_items(ctx(), max_items, max_item_members) == 0 }
    }
    /// What the span kernel decides for one item (pure: no GPU): `(complement mask, entries of the direct list, entries of the missing list)`, `None` for
    /// arguments the C entry refuses.
    pub fn plan_span(sizes: &[u32], eligible: &[bool], bits: &[u8], mode: i32) -> Option<(u64, u32, u32)> {
        assert!(sizes.len() == eligible.len());
        let el: Vec<u8> = eligible.iter().map(|&e| e as u8).collect();
        let (mut mask, mut nd, mut nm) = (0u64, 0u32, 0u32);
        let rc = unsafe {
            mbls_plan_committee_span(sizes.as_ptr(), el.as_ptr(), sizes.len() as u32, bits.as_ptr(), bits.len() as u32, mode as c_int, &mut mask, &mut nd, &mut nm)
        };
        if rc == 0 { Some((mask, nd, nm)) } else { None }
    }
    /// `AggregateSignature::verify_multiple_aggregate_signatures` over a gossip batch whose keys and messages are resident
    /// (`mbls_verify_multiple_committee_msgtable_rng`): every set is a signature, a `GossipKeys` -- a committee of this table with its participation bits, or ONE
    /// key of the key table the committees are bound to -- and an entry index of `table`. The same bool as that function on the spelled-out aggregate keys and
    /// messages, `rng` left in the same state. A committee id, key index or entry index that names nothing gives false.
    pub fn verify_multiple_aggregate_signatures<'a, R, I>(&self, rng: &mut R, signature_sets: I, table: &MessageTable) -> bool
    where
        R: Rng + ?Sized,
        I: Iterator<Item = (&'a AggregateSignature, GossipKeys<'a>, u32)>,
    {
        self.vm_committee(rng, signature_sets, table, false).0
    }
    /// The same, and in the same call (`mbls_verify_multiple_committee_msgtable_locate_rng`) which sets of a rejected call are the bad ones, with the semantics of
    /// `AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs_locate`.
    pub fn verify_multiple_aggregate_signatures_locate<'a, R, I>(&self, rng: &mut R, signature_sets: I, table: &MessageTable) -> (bool, Vec<bool>)
    where
        R: Rng + ?Sized,
        I: Iterator<Item = (&'a AggregateSignature, GossipKeys<'a>, u32)>,
    {
        self.vm_committee(rng, signature_sets, table, true)
    }
    fn vm_committee<'a, R, I>(&self, rng: &mut R, signature_sets: I, table: &MessageTable, locate: bool) -> (bool, Vec<bool>)
    where
        R: Rng + ?Sized,
        I: Iterator<Item = (&'a AggregateSignature, GossipKeys<'a>, u32)>,
    {
        let sets: Vec<(&AggregateSignature, GossipKeys, u32)> = signature_sets.collect();
        let n = sets.len();
        if n == 0 {
            return (true, Vec::new());
        }
        let mut sigs = Vec::new();
        let (mut words, mut idx): (Vec<u32>, Vec<u32>) = (Vec::with_capacity(n), Vec::with_capacity(n));
        let mut fields: Vec<&[u8]> = Vec::with_capacity(n);
        for (s, k, j) in &sets {
            sigs.extend_from_slice(&s.point);
            match *k {
                GossipKeys::Committee { id, bits } => {
                    assert!(id & VM_SET_SINGLE_KEY == 0, "committee ids have 31 bits");
                    words.push(id);
                    fields.push(bits);
                }
                GossipKeys::SingleKey(index) => {
                    assert!(index & VM_SET_SINGLE_KEY == 0, "key indices have 31 bits");
                    words.push(VM_SET_SINGLE_KEY | index);
                    fields.push(&[]);
                }
            }
            idx.push(*j);
        }
        let (flat, stride) = self.flatten_bits(&fields);
        let mut st = DrawState { rng, panic: None };
        let mut ok: u8 = 0;
        let mut sres: Vec<u8> = vec![0; if locate { n } else { 0 }];
        let rc = unsafe {
            if locate {
                mbls_verify_multiple_committee_msgtable_locate_rng(ctx(), self.h, sigs.as_ptr(), words.as_ptr(), flat.as_ptr(), stride, table.h, idx.as_ptr(), n as u64, &mut ok,
                                                                   sres.as_mut_ptr(), std::ptr::null_mut(), draw_scalars::<R>, &mut st as *mut DrawState<R> as *mut c_void)
            } else {
                mbls_verify_multiple_committee_msgtable_rng(ctx(), self.h, sigs.as_ptr(), words.as_ptr(), flat.as_ptr(), stride, table.h, idx.as_ptr(), n as u64, &mut ok,
                                                            draw_scalars::<R>, &mut st as *mut DrawState<R> as *mut c_void)
            }
        };
        if let Some(payload) = st.panic.take() {
            std::panic::resume_unwind(payload);
        }
        (rc == 0 && ok == 1, sres.iter().map(|&b| rc == 0 && b == 1).collect())
    }
    /// `verify_multiple_aggregate_signatures` once per batch, in order, as ONE call on the GPU (`mbls_verify_multiple_batches_committee_msgtable_rng`): one bool per
    /// batch, a bad batch rejects itself and nothing else, and the sets of a batch that name one entry of `table` share one Miller loop. `rng` is left where the
    /// per-batch calls would leave it. A committee id, key index or entry index that names nothing gives false for every batch.
    pub fn verify_multiple_aggregate_signatures_batches<'a, R>(&self, rng: &mut R, batches: &[Vec<(&'a AggregateSignature, GossipKeys<'a>, u32)>],
                                                               table: &MessageTable) -> Vec<bool>
    where
        R: Rng + ?Sized,
    {
        self.vm_committee_batches(rng, batches, table, false).0
    }
    /// The same, and in the same call (`mbls_verify_multiple_batches_committee_msgtable_locate_rng`) which sets of the rejected batches are the bad ones: per batch
    /// one bool per set, with the semantics of `AggregateSignature::verify_multiple_aggregate_signatures_batches_locate`.
    pub fn verify_multiple_aggregate_signatures_batches_locate<'a, R>(&self, rng: &mut R, batches: &[Vec<(&'a AggregateSignature, GossipKeys<'a>, u32)>],
                                                                      table: &MessageTable) -> (Vec<bool>, Vec<Vec<bool>>)
    where
        R: Rng + ?Sized,
    {
        self.vm_committee_batches(rng, batches, table, true)
    }
    fn vm_committee_batches<'a, R>(&self, rng: &mut R, batches: &[Vec<(&'a AggregateSignature, GossipKeys<'a>, u32)>], table: &MessageTable,
                                   locate: bool) -> (Vec<bool>, Vec<Vec<bool>>)
    where
        R: Rng + ?Sized,
    {
        let nb = batches.len();
        if nb == 0 {
            return (Vec::new(), Vec::new());
        }
        let n: usize = batches.iter().map(|b| b.len()).sum();
        let mut boff: Vec<u32> = Vec::with_capacity(nb + 1);
        boff.push(0);
        let mut sigs = Vec::new();
        let (mut words, mut idx): (Vec<u32>, Vec<u32>) = (Vec::with_capacity(n), Vec::with_capacity(n));
        let mut fields: Vec<&[u8]> = Vec::with_capacity(n);
        for b in batches {
            for (s, k, j) in b {
                sigs.extend_from_slice(&s.point);
                match *k {
                    GossipKeys::Committee { id, bits } => {
                        assert!(id & VM_SET_SINGLE_KEY == 0, "committee ids have 31 bits");
                        words.push(id);
                        fields.push(bits);
                    }
                    GossipKeys::SingleKey(index) => {
                        assert!(index & VM_SET_SINGLE_KEY == 0, "key indices have 31 bits");
                        words.push(VM_SET_SINGLE_KEY | index);
                        fields.push(&[]);
                    }
                }
                idx.push(*j);
            }
            boff.push(idx.len() as u32);
        }
        let (flat, stride) = self.flatten_bits(&fields);
        let mut st = DrawState { rng, panic: None };
        let mut res: Vec<u8> = vec![0; nb];
        let mut sres: Vec<u8> = vec![if n == 0 { 1 } else { 0 }; if locate { n.max(1) } else { 0 }];
        let rc = unsafe {
            if locate {
                mbls_verify_multiple_batches_committee_msgtable_locate_rng(ctx(), self.h, sigs.as_ptr(), words.as_ptr(), flat.as_ptr(), stride, table.h, idx.as_ptr(), n as u64,
                                                                           boff.as_ptr(), 0, nb as u64, res.as_mut_ptr(), sres.as_mut_ptr(), std::ptr::null_mut(),
                                                                           draw_scalars::<R>, &mut st as *mut DrawState<R> as *mut c_void)
            } else {
                mbls_verify_multiple_batches_committee_msgtable_rng(ctx(), self.h, sigs.as_ptr(), words.as_ptr(), flat.as_ptr(), stride, table.h, idx.as_ptr(), n as u64,
                                                                    boff.as_ptr(), 0, nb as u64, res.as_mut_ptr(), draw_scalars::<R>,
                                                                    &mut st as *mut DrawState<R> as *mut c_void)
            }
        };
        if let Some(payload) = st.panic.take() {
            std::panic::resume_unwind(payload);
        }
        let out: Vec<bool> = res.iter().map(|&b| rc == 0 && b == 1).collect();
        let per_set: Vec<Vec<bool>> = if locate {
            (0..nb).map(|b| sres[boff[b] as usize..boff[b + 1] as usize].iter().map(|&x| rc == 0 && x == 1).collect()).collect()
        } else {
            Vec::new()
        };
        (out, per_set)
    }
    /// `AggregateSignature::verify_multiple_aggregate_signatures` over a block's sets (`mbls_verify_multiple_committee_span_msgtable_rng`): every set is a
    /// signature, a `SpanKeys` -- the committees an attestation names with ONE field over their concatenated members, or ONE key of the key table -- and an entry
    /// index of `table`. The same bool as that function on the spelled-out aggregate keys and messages, `rng` left in the same state. A malformed set, a key index
    /// or an entry index that names nothing gives false.
    pub fn verify_multiple_aggregate_signatures_spans<'a, R, I>(&self, rng: &mut R, signature_sets: I, table: &MessageTable) -> bool
    where
        R: Rng + ?Sized,
        I: Iterator<Item = (&'a AggregateSignature, SpanKeys<'a>, u32)>,
    {
        self.vm_committee_span(rng, signature_sets, table, false).0
    }
    /// The same, and in the same call (`mbls_verify_multiple_committee_span_msgtable_locate_rng`) which sets of a rejected call are the bad ones.
    pub fn verify_multiple_aggregate_signatures_spans_locate<'a, R, I>(&self, rng: &mut R, signature_sets: I, table: &MessageTable) -> (bool, Vec<bool>)
    where
        R: Rng + ?Sized,
        I: Iterator<Item = (&'a AggregateSignature, SpanKeys<'a>, u32)>,
    {
        self.vm_committee_span(rng, signature_sets, table, true)
    }
    fn vm_committee_span<'a, R, I>(&self, rng: &mut R, signature_sets: I, table: &MessageTable, locate: bool) -> (bool, Vec<bool>)
    where
        R: Rng + ?Sized,
        I: Iterator<Item = (&'a AggregateSignature, SpanKeys<'a>, u32)>,
    {
        let sets: Vec<(&AggregateSignature, SpanKeys, u32)> = signature_sets.collect();
        let n = sets.len();
        if n == 0 {
            return (true, Vec::new());
        }
        let mut sigs = Vec::new();
        let (mut ids, mut off, mut idx): (Vec<u32>, Vec<u32>, Vec<u32>) = (Vec::new(), vec![0], Vec::with_capacity(n));
        let mut fields: Vec<&[u8]> = Vec::with_capacity(n);
        for (s, k, j) in &sets {
            sigs.extend_from_slice(&s.point);
            match *k {
                SpanKeys::Committees { ids: c, bits } => {
                    assert!(c.iter().all(|id| id & VM_SET_SINGLE_KEY == 0), "committee ids have 31 bits");
                    ids.extend_from_slice(c);
                    fields.push(bits);
                }
                SpanKeys::SingleKey(index) => {
                    assert!(index & VM_SET_SINGLE_KEY == 0, "key indices have 31 bits");
                    ids.push(VM_SET_SINGLE_KEY | index);
                    fields.push(&[]);
                }
            }
            off.push(ids.len() as u32);
            idx.push(*j);
        }
        let stride = ((fields.iter().map(|f| f.len()).max().unwrap_or(0).max(1) + 3) / 4 * 4) as u32;        // one stride for every field, a multiple of 4
        let mut flat = vec![0u8; stride as usize * n];
        for (i, f) in fields.iter().enumerate() {
            flat[stride as usize * i..stride as usize * i + f.len()].copy_from_slice(f);
        }
        let n_ids = ids.len() as u64;
        if ids.is_empty() {
            ids.push(0);
        }
        let mut st = DrawState { rng, panic: None };
        let mut ok: u8 = 0;
        let mut sres: Vec<u8> = vec![0; if locate { n } else { 0 }];
        let rc = unsafe {
            if locate {
                mbls_verify_multiple_committee_span_msgtable_locate_rng(ctx(), self.h, sigs.as_ptr(), ids.as_ptr(), n_ids, off.as_ptr(), flat.as_ptr(), stride, table.h,
                                                                        idx.as_ptr(), n as u64, &mut ok, sres.as_mut_ptr(), std::ptr::null_mut(), draw_scalars::<R>,
                                                                        &mut st as *mut DrawState<R> as *mut c_void)
            } else {
                mbls_verify_multiple_committee_span_msgtable_rng(ctx(), self.h, sigs.as_ptr(), ids.as_ptr(), n_ids, off.as_ptr(), flat.as_ptr(), stride, table.h, idx.as_ptr(),
                                                                 n as u64, &mut ok, draw_scalars::<R>, &mut st as *mut DrawState<R> as *mut c_void)
            }
        };
        if let Some(payload) = st.panic.take() {
            std::panic::resume_unwind(payload);
        }
        (rc == 0 && ok == 1, sres.iter().map(|&b| rc == 0 && b == 1).collect())
    }
    /// `verify_multiple_aggregate_signatures_spans` once per batch (per block), in order, as ONE call on the GPU
    /// (`mbls_verify_multiple_batches_committee_span_msgtable_rng`): one bool per batch, a bad batch rejects itself and nothing else. `rng` is left where the
    /// per-batch calls would leave it. A malformed set, a key index or an entry index that names nothing gives false for every batch.
    pub fn verify_multiple_aggregate_signatures_spans_batches<'a, R>(&self, rng: &mut R, batches: &[Vec<(&'a AggregateSignature, SpanKeys<'a>, u32)>],
                                                                     table: &MessageTable) -> Vec<bool>
    where
        R: Rng + ?Sized,
    {
        self.vm_committee_span_batches(rng, batches, table, false).0
    }
    /// The same, and in the same call (`mbls_verify_multiple_batches_committee_span_msgtable_locate_rng`) which sets of the rejected batches are the bad ones.
    pub fn verify_multiple_aggregate_signatures_spans_batches_locate<'a, R>(&self, rng: &mut R, batches: &[Vec<(&'a AggregateSignature, SpanKeys<'a>, u32)>],
                                                                            table: &MessageTable) -> (Vec<bool>, Vec<Vec<bool>>)
    where
        R: Rng + ?Sized,
    {
        self.vm_committee_span_batches(rng, batches, table, true)
    }
    fn vm_committee_span_batches<'a, R>(&self, rng: &mut R, batches: &[Vec<(&'a AggregateSignature, SpanKeys<'a>, u32)>], table: &MessageTable,
                                        locate: bool) -> (Vec<bool>, Vec<Vec<bool>>)
    where
        R: Rng + ?Sized,
    {
        let nb = batches.len();
        if nb == 0 {
            return (Vec::new(), Vec::new());
        }
        let n: usize = batches.iter().map(|b| b.len()).sum();
        let mut boff: Vec<u32> = Vec::with_capacity(nb + 1);
        boff.push(0);
        let mut sigs = Vec::new();
        let (mut ids, mut off, mut idx): (Vec<u32>, Vec<u32>, Vec<u32>) = (Vec::new(), vec![0], Vec::with_capacity(n));
        let mut fields: Vec<&[u8]> = Vec::with_capacity(n);
        for b in batches {
            for (s, k, j) in b {
                sigs.extend_from_slice(&s.point);
                match *k {
                    SpanKeys::Committees { ids: c, bits } => {
                        assert!(c.iter().all(|id| id & VM_SET_SINGLE_KEY == 0), "committee ids have 31 bits");
                        ids.extend_from_slice(c);
                        fields.push(bits);
                    }
                    SpanKeys::SingleKey(index) => {
                        assert!(index & VM_SET_SINGLE_KEY == 0, "key indices have 31 bits");
                        ids.push(VM_SET_SINGLE_KEY | index);
                        fields.push(&[]);
                    }
                }
                off.push(ids.len() as u32);
                idx.push(*j);
            }
            boff.push(idx.len() as u32);
        }
        let stride = ((fields.iter().map(|f| f.len()).max().unwrap_or(0).max(1) + 3) / 4 * 4) as u32;        // one stride for every field, a multiple of 4
        let mut flat = vec![0u8; stride as usize * n];
        for (i, f) in fields.iter().enumerate() {
            flat[stride as usize * i..stride as usize * i + f.len()].copy_from_slice(f);
        }
        let n_ids = ids.len() as u64;
        if ids.is_empty() {
            ids.push(0);
        }
        let mut st = DrawState { rng, panic: None };
        let mut res: Vec<u8> = vec![0; nb];
        let mut sres: Vec<u8> = vec![if n == 0 { 1 } else { 0 }; if locate { n.max(1) } else { 0 }];
        let rc = unsafe {
            if locate {
                mbls_verify_multiple_batches_committee_span_msgtable_locate_rng(ctx(), self.h, sigs.as_ptr(), ids.as_ptr(), n_ids, off.as_ptr(), flat.as_ptr(), stride,
                                                                                table.h, idx.as_ptr(), n as u64, boff.as_ptr(), 0, nb as u64, res.as_mut_ptr(),
                                                                                sres.as_mut_ptr(), std::ptr::null_mut(), draw_scalars::<R>,
                                                                                &mut st as *mut DrawState<R> as *mut c_void)
            } else {
                mbls_verify_multiple_batches_committee_span_msgtable_rng(ctx(), self.h, sigs.as_ptr(), ids.as_ptr(), n_ids, off.as_ptr(), flat.as_ptr(), stride, table.h,
                                                                         idx.as_ptr(), n as u64, boff.as_ptr(), 0, nb as u64, res.as_mut_ptr(), draw_scalars::<R>,
                                                                         &mut st as *mut DrawState<R> as *mut c_void)
            }
        };
        if let Some(payload) = st.panic.take() {
            std::panic::resume_unwind(payload);
        }
        let out: Vec<bool> = res.iter().map(|&b| rc == 0 && b == 1).collect();
        let per_set: Vec<Vec<bool>> = if locate {
            (0..nb).map(|b| sres[boff[b] as usize..boff[b + 1] as usize].iter().map(|&x| rc == 0 && x == 1).collect()).collect()
        } else {
            Vec::new()
        };
        (out, per_set)
    }
    /// The split factor of the key phase of the span form above: 0 auto, else 1, 2, 4, 8 or 16 lanes per key list (`mbls_ctx_set_vm_span_split`).
    pub fn set_vm_span_split(mode: u32) -> bool {
        unsafe { mbls_ctx_set_vm_span_split(ctx(), mode as c_int) == 0 }
    }
    /// What a call of the span form over `n` sets takes, without a GPU (`mbls_plan_verify_multiple_span`): (split factor, workspace items).
    pub fn plan_verify_multiple_spans(limits: &mbls_limits, n: u64, table_size: u64, stride_words: u64, locate: bool, split_mode: u32) -> Option<(u32, u64)> {
        let (mut split, mut items) = (0u32, 0u64);
        let rc = unsafe { mbls_plan_verify_multiple_span(limits, n, table_size, stride_words, locate as c_int, split_mode as c_int, &mut split, &mut items) };
        if rc == 0 { Some((split, items)) } else { None }
    }
}
/// The keys of one set of `CommitteeTable::verify_multiple_aggregate_signatures_spans`.
#[derive(Clone, Copy)]
pub enum SpanKeys<'a> {
    /// the selected members of the committees `ids` (at most `SPAN_MAX_COMMITTEES`), `bits` ONE field over their concatenated members (SSZ bit order)
    Committees { ids: &'a [u32], bits: &'a [u8] },
    /// entry `index` of the key table the committee table is bound to: a proposer signature, a randao reveal, an exit
    SingleKey(u32),
}
/// `MBLS_VM_SET_SINGLE_KEY` of include/mbls.h: bit 31 of a set's descriptor word marks a set under one key of the key table.
pub const VM_SET_SINGLE_KEY: u32 = 0x8000_0000;
/// `MBLS_SPAN_MAX_COMMITTEES`: the committees one item of the span entries may name (the protocol's MAX_COMMITTEES_PER_SLOT).
pub const SPAN_MAX_COMMITTEES: usize = 64;
/// The keys of one set of `CommitteeTable::verify_multiple_aggregate_signatures`.
#[derive(Clone, Copy)]
pub enum GossipKeys<'a> {
    /// the members of committee `id` whose bit is set in `bits` (SSZ bit order; bits at or above the committee's size are ignored)
    Committee { id: u32, bits: &'a [u8] },
    /// entry `index` of the key table the committee table is bound to: a selection proof, an aggregator's signature, an unaggregated attestation
    SingleKey(u32),
}
impl Drop for CommitteeTable {
    fn drop(&mut self) {
        unsafe { mbls_committees_destroy(self.h) }
    }
}
impl Drop for MessageTableStream {
    fn drop(&mut self) {
        unsafe { mbls_stream_destroy(self.h) }
    }
}
/// A verification stream over a `CommitteeTable` and a `MessageTable` (`mbls_stream_create_committee`): an item is a signature, an entry index, a committee id and
/// the committee's participation bits as SSZ serializes them; calls of any size, each with fields of its own byte length, are packed into full-round launches.
/// While the stream lives the committee table refuses a committee of more than `8 * bits_stride` members, and both tables refuse `clear` while calls are pending.
/// Drop the stream before both tables. (Like the rest of this crate: source only, never compiled.)
pub struct CommitteeStream {
    h: *mut mbls_stream,
    bits_stride: u32,
}
unsafe impl Send for CommitteeStream {}
unsafe impl Sync for CommitteeStream {}
impl CommitteeStream {
    /// `bits_stride`: a multiple of 4 with `8 * bits_stride` at least the table's largest committee
    pub fn new(committees: &mut CommitteeTable, table: &mut MessageTable, bits_stride: u32, opts: mbls_stream_opts) -> Self {
        let mut h: *mut mbls_stream = std::ptr::null_mut();
        let rc = unsafe { mbls_stream_create_committee(ctx(), committees.h, table.h, bits_stride, &opts, &mut h) };
        if rc != 0 {
            err(rc);
        }
        CommitteeStream { h, bits_stride }
    }
    /// n x fast_aggregate_verify: item i = (signatures[i], entry message_indices[i], the members of committee committee_ids[i] whose bit is set in bits[i]). The
    /// fields of one call travel at the length of its longest (at most `bits_stride` bytes); an id or an index that names nothing rejects its item.
    pub fn verify(&self, signatures: &[AggregateSignature], message_indices: &[u32], committee_ids: &[u32], bits: &[&[u8]]) -> Vec<bool> {
        let n = signatures.len();
        assert!(n > 0 && message_indices.len() == n && committee_ids.len() == n && bits.len() == n);
        let len = bits.iter().map(|b| b.len()).max().unwrap_or(1).max(1);
        assert!(len <= self.bits_stride as usize);
        let sigs: Vec<u8> = signatures.iter().flat_map(|s| s.point.iter().copied()).collect();
        let mut flat = vec![0u8; len * n];
        for (i, b) in bits.iter().enumerate() {
            flat[len * i..len * i + b.len()].copy_from_slice(b);
        }
        let mut res = vec![0u8; n];
        let mut ticket = 0u64;
        let mut rc = unsafe {
            mbls_stream_submit_committee(self.h, sigs.as_ptr(), message_indices.as_ptr(), committee_ids.as_ptr(), flat.as_ptr(), len as u32, n as u64, res.as_mut_ptr(),
                                         std::ptr::null_mut(), &mut ticket)
        };
        if rc == 0 {
            rc = unsafe { mbls_stream_wait(self.h, ticket) };       // the buffers above stay valid until the call completes
        }
        if rc != 0 {
            err(rc);
        }
        res.into_iter().map(|b| b == 1).collect()
    }
    pub fn flush(&self) {
        unsafe { mbls_stream_flush(self.h) };
    }
}
impl Drop for CommitteeStream {
    fn drop(&mut self) {
        unsafe { mbls_stream_destroy(self.h) }
    }
}
/// A verify_multiple stream over a `CommitteeTable` and a `MessageTable` (`mbls_stream_create_vm_committee`): many threads, each holding ONE small gossip batch.
/// A call is one batch and is never split; the stream packs the batches of many callers into one launch per round and answers per batch and per set. The
/// interlocks with the tables are `CommitteeStream`'s. Drop the stream before both tables. (Like the rest of this crate: source only, never compiled.)
pub struct VerifyMultipleStream {
    h: *mut mbls_stream,
    bits_stride: u32,
}
unsafe impl Send for VerifyMultipleStream {}
unsafe impl Sync for VerifyMultipleStream {}
impl VerifyMultipleStream {
    /// `bits_stride`: a multiple of 4 with `8 * bits_stride` at least the table's largest committee
    pub fn new(committees: &mut CommitteeTable, table: &mut MessageTable, bits_stride: u32, opts: mbls_stream_opts) -> Self {
        let mut h: *mut mbls_stream = std::ptr::null_mut();
        let rc = unsafe { mbls_stream_create_vm_committee(ctx(), committees.h, table.h, bits_stride, &opts, &mut h) };
        if rc != 0 {
            err(rc);
        }
        VerifyMultipleStream { h, bits_stride }
    }
    /// One batch of `CommitteeTable::verify_multiple_aggregate_signatures_locate`'s sets -> (the batch's bool, which sets of a rejected batch are good). One scalar
    /// per set is drawn from `rng` before the submit, in set order, by the reference's rule; unlike the `_rng` entries nothing is read back before the draw, so a
    /// batch with a signature outside G2 still consumes a scalar for every set. The fields travel at the length of the longest (at most `bits_stride` bytes; a
    /// batch of single-key sets only: 0). A committee id, key index or entry index that names nothing rejects the batch and names its set.
    pub fn verify<'a, R: Rng + ?Sized>(&self, rng: &mut R, sets: &[(&'a AggregateSignature, GossipKeys<'a>, u32)]) -> (bool, Vec<bool>) {
        let n = sets.len();
        assert!(n > 0);
        let mut sigs = Vec::new();
        let (mut words, mut idx, mut rands): (Vec<u32>, Vec<u32>, Vec<u64>) = (Vec::with_capacity(n), Vec::with_capacity(n), Vec::with_capacity(n));
        let mut fields: Vec<&[u8]> = Vec::with_capacity(n);
        for (s, k, j) in sets {
            sigs.extend_from_slice(&s.point);
            match *k {
                GossipKeys::Committee { id, bits } => {
                    assert!(id & VM_SET_SINGLE_KEY == 0, "committee ids have 31 bits");
                    words.push(id);
                    fields.push(bits);
                }
                GossipKeys::SingleKey(index) => {
                    assert!(index & VM_SET_SINGLE_KEY == 0, "key indices have 31 bits");
                    words.push(VM_SET_SINGLE_KEY | index);
                    fields.push(&[]);
                }
            }
            idx.push(*j);
            let mut rand = 0u64;
            while rand == 0 {
                let mut rand_bytes = [0u8; 8];
                rng.fill(&mut rand_bytes);
                rand = i64::from_be_bytes(rand_bytes).wrapping_abs() as u64;
            }
            rands.push(rand);
        }
        let len = fields.iter().map(|b| b.len()).max().unwrap_or(0);
        assert!(len <= self.bits_stride as usize);
        let mut flat = vec![0u8; len * n];
        for (i, b) in fields.iter().enumerate() {
            flat[len * i..len * i + b.len()].copy_from_slice(b);
        }
        let (mut ok, mut st, mut ticket) = (0u8, 0u32, 0u64);
        let mut sres = vec![0u8; n];
        let mut rc = unsafe {
            mbls_stream_submit_vm(self.h, sigs.as_ptr(), words.as_ptr(), if len > 0 { flat.as_ptr() } else { std::ptr::null() }, len as u32, idx.as_ptr(), rands.as_ptr(),
                                  n as u64, &mut ok, &mut st, sres.as_mut_ptr(), std::ptr::null_mut(), &mut ticket)
        };
        if rc == 0 {
            rc = unsafe { mbls_stream_wait(self.h, ticket) };       // the buffers above stay valid until the call completes
        }
        if rc != 0 {
            err(rc);
        }
        (ok == 1, sres.into_iter().map(|b| b == 1).collect())
    }
    pub fn flush(&self) {
        unsafe { mbls_stream_flush(self.h) };
    }
}
impl Drop for VerifyMultipleStream {
    fn drop(&mut self) {
        unsafe { mbls_stream_destroy(self.h) }
    }
}

#[allow(dead_code)]
fn _unused(_: *mut c_void) {}

#[cfg(test)]
mod tests {
    //! The reference's own unit tests that need no fixture files, restated (they need an MI355X to run).
    use super::*;

    #[test]
    fn test_readme_example() {
        // reference src/signature.rs:103-125
        let sk_bytes = [78, 252, 122, 126, 32, 0, 75, 89, 252, 31, 42, 130, 254, 88, 6, 90, 138, 202, 135, 194, 233, 117, 181, 75, 96, 238, 79, 100, 237, 59, 140, 111];
        let sk = SecretKey::from_bytes(&sk_bytes).unwrap();
        let pk = PublicKey::from_secret_key(&sk);
        let msg = "cats".as_bytes();
        let sig = Signature::new(msg, &sk);
        assert!(sig.verify(msg, &pk));
        assert!(!sig.verify("dogs".as_bytes(), &pk));
    }

    #[test]
    fn test_fast_aggregate_verify_infinity_aggregate_key() {
        // reference src/aggregates.rs:392-410: pk(1) + pk(r-1) = infinity -> false
        let mut one = [0u8; 32];
        one[31] = 1;
        let mut rm1 = CURVE_ORDER_BE;
        rm1[31] = 0;
        let sk1 = SecretKey::from_bytes(&one).unwrap();
        let sk2 = SecretKey::from_bytes(&rm1).unwrap();
        let (pk1, pk2) = (PublicKey::from_secret_key(&sk1), PublicKey::from_secret_key(&sk2));
        let msg = [1u8; 32];
        let mut agg = AggregateSignature::new();
        agg.add(&Signature::new(&msg, &sk1));
        agg.add(&Signature::new(&msg, &sk2));
        assert!(!agg.fast_aggregate_verify(&msg, &[&pk1, &pk2]));
        assert!(!AggregateSignature::new().fast_aggregate_verify(&msg, &[]));
    }
}

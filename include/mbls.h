/*
 * mbls.h -- C ABI of libmbls_hip.so: MI355X (gfx950) batch BLS12-381 signature verification.
 *
 * This is the drop-in boundary for the verification path of sigp/milagro_bls. The reference has no FFI of
 * its own (it is a Rust library over the `amcl` crate); these entry points are what a Rust shim re-creating
 * reference src/lib.rs:17-22 would bind. Each entry cites the reference interface it
 * replaces. Plain pointers and sizes only; the caller owns every buffer.
 *
 * Wire formats (ZCash BLS12-381 serialization, as in the reference):
 *   signature / aggregate signature : 96 bytes, compressed G2      (Signature::as_bytes, src/signature.rs:49-51)
 *   public key, compressed          : 48 bytes                      (PublicKey::as_bytes, src/keys.rs:158-160)
 *   public key, uncompressed        : 96 bytes x||y                 (PublicKey::as_uncompressed_bytes, src/keys.rs:163-165)
 *   secret key                      : 32 bytes big-endian           (SecretKey::as_bytes, src/keys.rs:85-87)
 * A decoded PublicKey / AggregatePublicKey object is represented by its 96-byte uncompressed form, a decoded
 * Signature / AggregateSignature by its 96-byte compressed form (amcl's in-memory layout is private).
 *
 * There is NO CPU fallback: every function runs HIP kernels and returns MBLS_ERR_DEVICE if the GPU is
 * unavailable. `*_device` variants take device pointers (inputs already resident in HBM) and a hipStream_t
 * (passed as void*); the others take host pointers and stage through the context's device buffers.
 */
#ifndef MBLS_H
#define MBLS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* error codes: the AmclError variants the reference uses (src/amcl_utils.rs:55,71; src/keys.rs:47,143,293;
   src/aggregates.rs:31) plus device errors */
#define MBLS_OK 0
#define MBLS_ERR_INVALID_G1_SIZE 1          /* AmclError::InvalidG1Size */
#define MBLS_ERR_INVALID_G2_SIZE 2          /* AmclError::InvalidG2Size */
#define MBLS_ERR_INVALID_POINT 3            /* AmclError::InvalidPoint */
#define MBLS_ERR_AGGREGATE_EMPTY_POINTS 4   /* AmclError::AggregateEmptyPoints */
#define MBLS_ERR_INVALID_SECRET_KEY_SIZE 5  /* AmclError::InvalidSecretKeySize */
#define MBLS_ERR_INVALID_SECRET_KEY_RANGE 6 /* AmclError::InvalidSecretKeyRange */
#define MBLS_ERR_DEVICE 100                 /* HIP failure / no GPU */
#define MBLS_ERR_ARGUMENT 101

#define MBLS_G1_BYTES 48                    /* reference src/lib.rs:20 G1_BYTES */
#define MBLS_G2_BYTES 96                    /* reference src/lib.rs:20 G2_BYTES */
#define MBLS_SECRET_KEY_BYTES 32            /* reference src/lib.rs:20 SECRET_KEY_BYTES */
#define MBLS_PK_COMPRESSED 0
#define MBLS_PK_UNCOMPRESSED 1

/* per-item status bits reported by the batch verifiers (why an item was rejected) */
#define MBLS_ST_BAD_SIG_ENCODING 0x01u
#define MBLS_ST_SIG_NOT_IN_G2 0x02u
#define MBLS_ST_BAD_PK_ENCODING 0x04u
#define MBLS_ST_APK_INFINITY 0x08u
#define MBLS_ST_NO_KEYS 0x10u
#define MBLS_ST_PK_INFINITY 0x20u
#define MBLS_ST_PAIRING_FAILED 0x40u
#define MBLS_ST_BAD_SCALAR 0x80u            /* verify_multiple: a zero blinding scalar */
#define MBLS_ST_BAD_MSG_RANGE 0x100u        /* msg_offsets[i+1] < msg_offsets[i] (device entries; host entries refuse the call) */

typedef struct mbls_ctx mbls_ctx;

/* ---- context: one per GPU (one process per GPU in multi-GPU runs) ----
 * Thread safety: every entry point takes the context's lock, so a context may be shared by any number of threads (the
 * reference's functions are pure and re-entrant); calls on one context run one after the other.
 * Device-pointer entries only enqueue work (none of them synchronises with the host): a later call on another stream waits
 * (on the device) for the workspace of the earlier one. For concurrent streams of work create one context per stream.
 * ONE EXCEPTION, by construction: a call whose batch is larger than any the context has seen first GROWS the workspace
 * (hipFree + hipMalloc inside mbls_ctx_reserve: both drain the device). Reserve the largest batch up front with
 * mbls_ctx_reserve / mbls_ctx_reserve_keys and no *_device entry ever synchronises. */
int mbls_ctx_create(mbls_ctx** out, int device_id);
void mbls_ctx_destroy(mbls_ctx* ctx);
/* pre-allocate the HBM workspace for batches of up to max_items items (6 384 bytes per item; avoids allocation in timed regions) */
int mbls_ctx_reserve(mbls_ctx* ctx, uint64_t max_items);
/* pre-allocate the staging area for max_keys decompressed public keys (compressed wire format, 96 bytes per key) */
int mbls_ctx_reserve_keys(mbls_ctx* ctx, uint64_t max_keys);
const char* mbls_last_error(mbls_ctx* ctx);
/* Small batches are latency-bound (one lane per item walks 14 M dependent instructions whatever the batch size), so batches of up to
 * max_items items run their pairing check -- Miller loop + final exponentiation -- with ONE WAVE per item, the item's field values
 * shared by the 64 lanes (mbls_coop.h); the message phase after hash_to_field does the same. Same results, bit for bit.
 * Defaults 5120 / 3584: the measured crossovers (between them the message phase runs on lane pairs; environment, read by mbls_ctx_create and therefore also by every context of an
 * mbls_multi handle: MBLS_COOP_MAX_ITEMS, MBLS_COOP_HASH_MAX_ITEMS); 0 = never. */
int mbls_ctx_set_coop_max_items(mbls_ctx* ctx, uint64_t max_items);
int mbls_ctx_reset_tuning(mbls_ctx* ctx);      /* every routing parameter of this section back to its default (environment overrides included) */
int mbls_ctx_set_coop_hash_max_items(mbls_ctx* ctx, uint64_t max_items);     /* the same for the message phase (never above the limit above) */
/* Within those limits, batches of pairing_min_items < n <= pairing_max_items items run the pairing check with two items per wave, and of
 * more than hash_min_items the message phase with four: more steps per wave, fewer per item -- it pays where it saves a round of waves.
 * Defaults (1024, 2048] and 768 (measured); min = UINT64_MAX: never. */
int mbls_ctx_set_coop_packing(mbls_ctx* ctx, uint64_t pairing_min_items, uint64_t pairing_max_items, uint64_t hash_min_items);
/* One ROUND of the one-lane-per-item kernels is one wave on every SIMD: CUs x 4 x 64 items (65 536 on MI355X; the kernels hold 512 registers
 * per lane, so a SIMD runs one wave at a time). A batch of q rounds + r items would cost q + 1 rounds of every kernel: the library runs the
 * q rounds and then the r items as a batch of their own, which takes the route of an r-item batch (one wave per item up to the limits
 * above). items = 0 restores the device's value; any multiple of 64 is accepted (tests use small rounds to exercise the cut). */
int mbls_ctx_set_round_items(mbls_ctx* ctx, uint64_t items);
/* Shaping of the one-lane path below a full round. Up to split_max_items items (default and maximum: half a round) the two pairs of an item's
 * Miller loop are walked on TWO lanes by the one-pair routine (6.6 ms instead of 11.3 ms; the product and the signature's subgroup verdict
 * follow as separate small kernels); up to fork_max_items items (default: three quarters of a round) the three front phases -- key sum, signature decoding,
 * message hashing -- are enqueued side by side on the context's own streams instead of one after the other. 0 = never. Same results, bit for
 * bit (environment for new contexts: MBLS_SPLIT_MAX_ITEMS, MBLS_FORK_MAX_ITEMS). */
int mbls_ctx_set_lane_shaping(mbls_ctx* ctx, uint64_t split_max_items, uint64_t fork_max_items);
/* Batches above a round, n = q rounds + r items. r < min_rest_items: the remainder follows the rounds as a batch of its own (mbls_ctx_set_round_items).
 * r >= min_rest_items: after the q - 1 whole rounds in front, the LAST round and the remainder run on TWO TRACKS side by side -- each on its own part of the
 * workspace and its own streams, so that the SIMDs one leaves idle take waves of the other --: up to side_max_items the round on one track and the remainder (on
 * the lane-pair forms, whatever its size) on the other, above it two equal halves of (round + r) / 2 items. Defaults 3 584 and a quarter of a round (measured:
 * 69 632 items 35.0 -> 33.7 ms, 73 728 items 40.0 -> 33.8 ms, 100 000 items 51.6 -> 46.5 ms); min_rest_items = 0: never. Same results, bit for bit (environment for new contexts:
 * MBLS_TRACKS_MIN_REST, MBLS_TRACKS_SIDE_MAX). */
int mbls_ctx_set_tracks(mbls_ctx* ctx, uint64_t min_rest_items, uint64_t side_max_items);
/* 0 (default): lookups that depend on a secret key are scans with selection; 1: the variable-time forms (see "SECRET KEYS ON THE DEVICE" below) */
int mbls_ctx_set_secret_ops(mbls_ctx* ctx, int variable_time);

/* ---- routing, as data (pure functions: no GPU, no context) -------------------------------------------------
 * Which kernels a batch of n items takes is decided by the limits above; mbls_plan_batch states the decision without running anything -- the SAME
 * function the verification entries call (verify_pipeline), so the table in DESIGN.md section 5 is checkable on a machine without a GPU
 * (tests/test_plan_cpu.py). mbls_default_limits fills the defaults for a device with round_items = CUs x 4 x 64 (65 536 on MI355X);
 * mbls_ctx_get_limits reads a context's current ones (setters and environment applied). The plan is a function of n alone; two forms follow from it and from
 * the keys per item: with the pairing check on waves (MBLS_PAIRING_WAVE*) the signature phase runs on lane pairs (k_sig2), and an item's key sum of k >= 32
 * keys, k a multiple of 8, uniform layout, as eight partial sums on lanes of their own (k_apk_combine; workspace n + 8 n items instead of workspace_items). */
typedef struct mbls_limits {
    uint64_t round_items, coop_max_items, coop_hash_max_items, coop_pack_min_items, coop_pack_max_items, coop_hash_pack_min_items,
             split_max_items, fork_max_items, hash2_max_items, tracks_min_rest, tracks_side_max;
} mbls_limits;
enum { MBLS_PAIRING_WAVE = 0,        /* one wave per item walks Miller loop + final exponentiation (program pairing2) */
       MBLS_PAIRING_WAVE_X2 = 5,     /* ... two items per wave (pairing2x2) */
       MBLS_PAIRING_LANE = 1,        /* one lane per item: k_miller (two-pair loop) + k_final -- the headline kernels */
       MBLS_PAIRING_LANES2 = 2,      /* two lanes per item: k_miller_split + k_final2 */
       MBLS_PAIRING_LANES4 = 4 };    /* four lanes per item in the Miller phase (k_miller_split4), two in the final exponentiation (k_final2) */
enum { MBLS_MESSAGE_LANE = 1, MBLS_MESSAGE_LANES2 = 2, MBLS_MESSAGE_WAVE = 3, MBLS_MESSAGE_WAVE_X4 = 4 };   /* k_hash / k_hash2 / hashg2 / hashg2x4 */
enum { MBLS_FRONT_IN_A_ROW = 0,      /* key sum -> signature -> message phase on one stream */
       MBLS_FRONT_MESSAGE_BESIDE = 1,/* message phase on a side stream beside key sum -> signature */
       MBLS_FRONT_ALL_BESIDE = 2 };  /* all three side by side */
typedef struct mbls_pass_plan {      /* one pass of the pipeline over a contiguous range of items */
    uint64_t first_item, items, workspace_first, workspace_items;
    uint32_t track;                  /* 0: the caller's stream; 1: the second track, side by side with track 0 of the same stage */
    uint32_t stage;                  /* passes of one stage run side by side, stages one after the other */
    uint32_t pairing, message, front, sig_subgroup_from_miller_loop;
} mbls_pass_plan;
enum { MBLS_BATCH_ONE_PASS = 0, MBLS_BATCH_ROUNDS_THEN_REST = 1, MBLS_BATCH_ROUND_BESIDE_REST = 2, MBLS_BATCH_TWO_HALVES = 3 };
typedef struct mbls_batch_plan { uint32_t mode, n_passes; mbls_pass_plan pass[3]; } mbls_batch_plan;
void mbls_default_limits(uint64_t round_items, mbls_limits* out);
int mbls_ctx_get_limits(mbls_ctx* ctx, mbls_limits* out);
/* the plan of mbls_fast_aggregate_verify_batch[_indexed]_device / mbls_verify_batch_device for n items (MBLS_ERR_ARGUMENT for n = 0 or null pointers) */
int mbls_plan_batch(const mbls_limits* limits, uint64_t n, mbls_batch_plan* out);
/* the workspace items that plan needs for items of k keys each -- split_layout != 0: uniform 96-byte keys (4-byte aligned) or key-table indices, the layouts whose
 * key sums on the wave engine take eight lanes per item (n + 8 n items for such a pass instead of its workspace_items). This is what the verification entries
 * reserve BEFORE they queue the first pass of a plan (no pass ever grows the workspace under another in flight); mbls_ctx_reserve(ctx, this) beforehand keeps
 * every allocation out of the call. 0 for n = 0 or a null pointer. */
uint64_t mbls_plan_workspace_items(const mbls_limits* limits, uint64_t n, uint32_t k, int split_layout);

/* ---- the hot path -------------------------------------------------------------------------------------
 * Batch of n independent AggregateSignature::fast_aggregate_verify calls (reference src/aggregates.rs:177-215):
 * item i = (sigs[96 i..], its message, its public keys). The reference takes any `msg: &[u8]` per call: messages are
 * either msg_len bytes each, contiguous (msg_offsets == NULL: item i's message is msgs[msg_len i ..]), or of any length
 * each: item i's message is msgs[msg_offsets[i] .. msg_offsets[i+1]) with msg_offsets of n + 1 non-decreasing entries
 * (msg_len is then ignored; host entries refuse a table that runs backwards or holds a message of 2^32 bytes or more,
 * device entries reject such an item with MBLS_ST_BAD_MSG_RANGE). Keys are either k per item, contiguous
 * (pk_offsets == NULL), or ragged: item i owns keys [pk_offsets[i], pk_offsets[i+1]) of `pks`.
 * results[i] = 1/0 exactly as the reference function returns true/false, including its check order:
 * empty key list -> 0, signature outside G2 -> 0, aggregate key = infinity -> 0, pairing check.
 * bitmap (optional, ceil(n/64) words): bit (i%64) of word i/64 = results[i]. status (optional): MBLS_ST_* bits. */
int mbls_fast_aggregate_verify_batch_device(mbls_ctx* ctx, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_len,
                                            const uint64_t* d_msg_offsets, const uint8_t* d_pks, int pk_format,
                                            const uint32_t* d_pk_offsets, uint64_t n, uint32_t k, uint8_t* d_results,
                                            uint64_t* d_bitmap, uint32_t* d_status, void* stream);
int mbls_fast_aggregate_verify_batch(mbls_ctx* ctx, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len,
                                     const uint64_t* msg_offsets, const uint8_t* pks, int pk_format,
                                     const uint32_t* pk_offsets, uint64_t n, uint32_t k, uint8_t* results, uint32_t* status);
/* Batch of n Signature::verify calls (reference src/signature.rs:27-40): one key per item, no infinity check. */
int mbls_verify_batch_device(mbls_ctx* ctx, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_len,
                             const uint64_t* d_msg_offsets, const uint8_t* d_pks, int pk_format, uint64_t n,
                             uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream);
int mbls_verify_batch(mbls_ctx* ctx, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* msg_offsets,
                      const uint8_t* pks, int pk_format, uint64_t n, uint8_t* results, uint32_t* status);

/* ---- resident key table ---------------------------------------------------------------------------------
 * The on-device analogue of the decoded PublicKey objects a reference caller keeps (src/keys.rs:116-120; callers cache
 * decoded keys through as_uncompressed_bytes / from_uncompressed_bytes, src/keys.rs:163-175): keys are decoded (and
 * optionally KeyValidate'd) ONCE into HBM as affine Montgomery limbs, and a verification names its keys by table index --
 * what `&[&PublicKey]` is in the reference's fast_aggregate_verify (src/aggregates.rs:177). Per use this removes the byte
 * decoding, the Montgomery conversion and the on-curve check (5 of 16 multiplications per key), makes the compressed
 * 48-byte wire format a one-time cost, and cuts the per-item input to 96 + msg_len + 4 k bytes.
 * A table belongs to the context it was created with (same GPU, same lock). Entries are never removed; indices are stable.
 * Ordering: an append made through mbls_keytable_append_device on one stream is seen by verifications and mbls_keytable_get on any
 * other stream (they wait for it on the device). Destroying the context first releases its tables' records; the handles stay
 * valid for mbls_keytable_destroy only. */
typedef struct mbls_keytable mbls_keytable;
int mbls_keytable_create(mbls_ctx* ctx, uint64_t capacity_hint, mbls_keytable** out);
void mbls_keytable_destroy(mbls_keytable* t);
uint64_t mbls_keytable_size(const mbls_keytable* t);
/* n x PublicKey::from_bytes (pk_format compressed, validate = 1), from_bytes_unchecked (compressed, 0) or
 * from_uncompressed_bytes (uncompressed, 0): entry first_index + i holds key i; errs[i] = MBLS_OK / MBLS_ERR_* exactly as
 * the reference constructor would return. A key that failed is stored as an invalid entry: every item that names it is
 * rejected with MBLS_ST_BAD_PK_ENCODING (the reference caller would hold no PublicKey to pass). */
int mbls_keytable_append(mbls_keytable* t, const uint8_t* pks, int pk_format, int validate, uint64_t n, uint64_t* first_index, uint8_t* errs);
int mbls_keytable_append_device(mbls_keytable* t, const uint8_t* d_pks, int pk_format, int validate, uint64_t n, uint64_t* first_index,
                                uint8_t* d_errs, void* stream);
/* PublicKey::as_uncompressed_bytes of n consecutive entries (src/keys.rs:163-165); errs[i] = MBLS_ERR_INVALID_POINT for invalid entries */
int mbls_keytable_get(mbls_keytable* t, uint64_t first_index, uint64_t n, uint8_t* pks96, uint8_t* errs);
/* The hot path over table indices: item i uses entries key_idx[k i .. k i + k) (offsets == NULL) or
 * key_idx[offsets[i] .. offsets[i+1]). An index >= mbls_keytable_size counts as an undecodable key. Same results, bitmap and
 * status words as mbls_fast_aggregate_verify_batch over the same keys in wire format. */
int mbls_fast_aggregate_verify_batch_indexed_device(mbls_ctx* ctx, const mbls_keytable* t, const uint8_t* d_sigs, const uint8_t* d_msgs,
                                                    uint32_t msg_len, const uint64_t* d_msg_offsets, const uint32_t* d_key_idx,
                                                    const uint32_t* d_offsets, uint64_t n, uint32_t k,
                                                    uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream);
int mbls_fast_aggregate_verify_batch_indexed(mbls_ctx* ctx, const mbls_keytable* t, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len,
                                             const uint64_t* msg_offsets, const uint32_t* key_idx, const uint32_t* offsets, uint64_t n,
                                             uint32_t k, uint8_t* results, uint32_t* status);

/* ---- shared message lists: hash each distinct message once ------------------------------------------------
 * The members of a committee sign the same message: a slot's gossip is tens of thousands of signatures over a few hundred distinct signing roots, and a batch
 * that spells the message out per item hashes every one of them to G2 (the second largest kernel of the full round). These entries are the message side's
 * counterpart of the key table: the call carries a LIST of n_msgs messages -- msg_len bytes each, or message j = msgs[msg_offsets[j] .. msg_offsets[j+1]) with a
 * table of n_msgs + 1 entries -- and one uint32 per item: item i's message is message msg_idx[i]. The list is hashed once, in the form ITS size asks for (a few
 * hundred messages take the wave engine whatever n is), and the message phase of every item is a 288-byte copy. results[i], status[i] and the bitmap are exactly
 * what the entry without `_shared_msgs` returns for the same signatures and keys with item i's message spelled out. n_msgs may be smaller than, equal to or larger
 * than n (unused messages are hashed and ignored); n = 0 returns MBLS_OK with nothing written.
 * DEVICE ENTRIES (enqueue only; ordered against other users of the workspace like their neighbours): msg_idx[i] >= n_msgs (n_msgs = 0 included) rejects item i
 * with MBLS_ST_BAD_MSG_RANGE and result 0; a listed message whose range runs backwards or is 2^32 bytes or more rejects every item that names it and nothing else.
 * Neither becomes a read outside the call's buffers; such items check against H of the empty message, like the bad-range items of the per-item entries.
 * HOST ENTRIES refuse a bad offset table, or an index >= n_msgs, with MBLS_ERR_ARGUMENT before anything is enqueued (results and status are left unwritten).
 * ALLOCATION: the hashed points live in a table of the context (288 bytes per message), and the list is hashed in the call's workspace: a call whose list is
 * larger than any before grows them first (which drains the device, see mbls_ctx_reserve). mbls_ctx_reserve_msgs(ctx, max_msgs) and
 * mbls_ctx_reserve(ctx, mbls_plan_shared_msgs_workspace_items(...)) beforehand keep every allocation out of the call.
 * A list that outlives the call, for many calls and for the verification stream: the resident message table below (mbls_msgtable_*). */
int mbls_ctx_reserve_msgs(mbls_ctx* ctx, uint64_t max_msgs);
/* Routing as data (pure: no GPU, no context), beside mbls_plan_batch: `batch` is mbls_plan_batch(limits, n) with the message phase of every pass marked
 * MBLS_MESSAGE_GATHER; the list of n_msgs messages is hashed in list_pieces pieces of list_piece_items messages (the last may be shorter; a piece is at most one
 * round), in the form list_message (MBLS_MESSAGE_*, chosen by the size of a piece, not by n), message j of a piece in workspace item j of list_workspace_items
 * (two per message on lane pairs). A plan of one pass hashes the list on the pass's message stream, beside its key sum and signature phases; a plan of several
 * passes hashes it once, before the first. table_entries = n_msgs + 1 (the empty message's entry). n_msgs = 0: no pieces, list_message = 0. The SAME function
 * the shared-message entries act on. MBLS_ERR_ARGUMENT for n = 0 or null pointers. */
enum { MBLS_MESSAGE_GATHER = 5 };      /* k_h_gather: the item copies its message's point from the context's table */
typedef struct mbls_shared_msgs_plan {
    mbls_batch_plan batch;
    uint32_t list_message, list_pieces;
    uint64_t list_piece_items, list_workspace_items, table_entries;
} mbls_shared_msgs_plan;
int mbls_plan_batch_shared_msgs(const mbls_limits* limits, uint64_t n, uint64_t n_msgs, mbls_shared_msgs_plan* out);
/* the workspace items such a call reserves before it queues anything: the larger of mbls_plan_workspace_items(limits, n, k, split_layout) and list_workspace_items */
uint64_t mbls_plan_shared_msgs_workspace_items(const mbls_limits* limits, uint64_t n, uint64_t n_msgs, uint32_t k, int split_layout);
/* mbls_fast_aggregate_verify_batch[_device] over a message list */
int mbls_fast_aggregate_verify_batch_shared_msgs_device(mbls_ctx* ctx, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_len,
                                                        const uint64_t* d_msg_offsets, uint64_t n_msgs, const uint32_t* d_msg_idx, const uint8_t* d_pks,
                                                        int pk_format, const uint32_t* d_pk_offsets, uint64_t n, uint32_t k, uint8_t* d_results,
                                                        uint64_t* d_bitmap, uint32_t* d_status, void* stream);
int mbls_fast_aggregate_verify_batch_shared_msgs(mbls_ctx* ctx, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* msg_offsets,
                                                 uint64_t n_msgs, const uint32_t* msg_idx, const uint8_t* pks, int pk_format, const uint32_t* pk_offsets,
                                                 uint64_t n, uint32_t k, uint8_t* results, uint32_t* status);
/* mbls_verify_batch[_device] over a message list */
int mbls_verify_batch_shared_msgs_device(mbls_ctx* ctx, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_msg_offsets,
                                         uint64_t n_msgs, const uint32_t* d_msg_idx, const uint8_t* d_pks, int pk_format, uint64_t n,
                                         uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream);
int mbls_verify_batch_shared_msgs(mbls_ctx* ctx, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* msg_offsets, uint64_t n_msgs,
                                  const uint32_t* msg_idx, const uint8_t* pks, int pk_format, uint64_t n, uint8_t* results, uint32_t* status);
/* mbls_fast_aggregate_verify_batch_indexed[_device] over a message list: keys by table index, messages by list index */
int mbls_fast_aggregate_verify_batch_indexed_shared_msgs_device(mbls_ctx* ctx, const mbls_keytable* t, const uint8_t* d_sigs, const uint8_t* d_msgs,
                                                                uint32_t msg_len, const uint64_t* d_msg_offsets, uint64_t n_msgs, const uint32_t* d_msg_idx,
                                                                const uint32_t* d_key_idx, const uint32_t* d_offsets, uint64_t n, uint32_t k,
                                                                uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream);
int mbls_fast_aggregate_verify_batch_indexed_shared_msgs(mbls_ctx* ctx, const mbls_keytable* t, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len,
                                                         const uint64_t* msg_offsets, uint64_t n_msgs, const uint32_t* msg_idx, const uint32_t* key_idx,
                                                         const uint32_t* offsets, uint64_t n, uint32_t k, uint8_t* results, uint32_t* status);

/* ---- resident message table: hash a message once, verify against it in any call or stream ------------------
 * The message side's key table. A slot's gossip arrives in hundreds of small calls over the same few hundred signing roots: the shared lists above hash a
 * call's list once per CALL, this table hashes a message once. Entry first_index + j holds H(message j) -- the 72 dwords of the hashed point and the message's
 * bad-range bit, exactly what a shared list's export writes -- and verifications name entries by index, in any later call, on any stream, and in a verification
 * stream (mbls_stream_create_msgtable). Public indices start at 0 and never change; entries are never rewritten. The table keeps a private entry for the empty
 * message: what an index that names nothing is checked against.
 * APPEND hashes in the form the COUNT of appended messages asks for (the list rule of mbls_plan_batch_shared_msgs: pieces of at most one round; wave engine,
 *   lane pairs or one lane per message), works in the context's workspace (ordered against its other users like any call; mbls_ctx_reserve beforehand keeps the
 *   allocation out of it) and exports at first_index. Messages as everywhere: msg_len bytes each, or message j = msgs[msg_offsets[j] .. msg_offsets[j+1]) with
 *   n + 1 offsets. The host form refuses a bad offset table with MBLS_ERR_ARGUMENT; in the device form a message whose range runs backwards or is 2^32 bytes or
 *   more becomes a FLAGGED entry, which rejects exactly the items that name it, with MBLS_ST_BAD_MSG_RANGE. n = 0 is MBLS_OK with *first_index = size.
 * ORDERING is the key table's: an append enqueued on one stream is seen by verifications, mbls_msgtable_get and later appends on any other stream (they wait
 *   for it on the device).
 * GROWTH. A table created with a sufficient capacity_hint (0: 1 024) never allocates again. Growth beyond it keeps every index and entry; it drains the device,
 *   as mbls_ctx_reserve does (the layout is entry-major with stride = capacity + 1, so growth moves every entry: csrc/mbls_mtb.h).
 * mbls_msgtable_get returns the compressed points of n entries in the format of mbls_hash_to_g2_batch; errs[i] = MBLS_ERR_ARGUMENT for a flagged entry.
 * mbls_msgtable_clear blocks until everything enqueued that reads the table has finished, then sets the size to 0 and keeps the capacity (index 0 names the
 *   next message appended). It is refused with MBLS_ERR_ARGUMENT (reason in mbls_last_error) while a stream bound to the table has calls that have not
 *   completed. The intended use is two tables alternated per slot or epoch.
 * LIFETIME. Destroy a table after the streams bound to it and before its context (a table whose context went first is an empty shell that only
 *   mbls_msgtable_destroy accepts). A table of another context is refused everywhere.
 * VERIFICATION ENTRIES. Each is its `_shared_msgs` neighbour with the list arguments (msgs, msg_len, msg_offsets, n_msgs) replaced by the table; msg_idx stays,
 *   one uint32 per item. No list is hashed. ROUTING: mbls_plan_batch(limits, n) with the message phase of every pass MBLS_MESSAGE_GATHER -- that is
 *   mbls_plan_batch_shared_msgs(limits, n, 0).batch --, in every plan shape; the workspace is mbls_plan_workspace_items. results[i], status[i] and the bitmap are
 *   bit for bit what the per-item entry returns with item i's message spelled out. The table is read at the size it has when the call is enqueued: in the device
 *   forms msg_idx[i] >= size (an empty table included) rejects item i with MBLS_ST_BAD_MSG_RANGE and result 0, checked against the empty message's point -- never
 *   a read outside the table; the host forms refuse such an index with MBLS_ERR_ARGUMENT before anything is enqueued and leave the outputs unwritten.
 * OUT OF SCOPE: verify_multiple over a resident table (the grouped route sizes its group arrays by the list), the mbls_multi handle, and device-side
 *   deduplication (callers intern their messages on the host). */
typedef struct mbls_msgtable mbls_msgtable;
int mbls_msgtable_create(mbls_ctx* ctx, uint64_t capacity_hint, mbls_msgtable** out);
void mbls_msgtable_destroy(mbls_msgtable* t);
uint64_t mbls_msgtable_size(const mbls_msgtable* t);
int mbls_msgtable_append(mbls_msgtable* t, const uint8_t* msgs, uint32_t msg_len, const uint64_t* msg_offsets, uint64_t n, uint64_t* first_index);
int mbls_msgtable_append_device(mbls_msgtable* t, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_msg_offsets, uint64_t n, uint64_t* first_index,
                                void* stream);
int mbls_msgtable_get(mbls_msgtable* t, uint64_t first_index, uint64_t n, uint8_t* out96, uint8_t* errs);
int mbls_msgtable_clear(mbls_msgtable* t);
int mbls_fast_aggregate_verify_batch_msgtable_device(mbls_ctx* ctx, const uint8_t* d_sigs, const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint8_t* d_pks,
                                                     int pk_format, const uint32_t* d_pk_offsets, uint64_t n, uint32_t k, uint8_t* d_results, uint64_t* d_bitmap,
                                                     uint32_t* d_status, void* stream);
int mbls_fast_aggregate_verify_batch_msgtable(mbls_ctx* ctx, const uint8_t* sigs, const mbls_msgtable* mt, const uint32_t* msg_idx, const uint8_t* pks, int pk_format,
                                              const uint32_t* pk_offsets, uint64_t n, uint32_t k, uint8_t* results, uint32_t* status);
int mbls_verify_batch_msgtable_device(mbls_ctx* ctx, const uint8_t* d_sigs, const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint8_t* d_pks, int pk_format,
                                      uint64_t n, uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream);
int mbls_verify_batch_msgtable(mbls_ctx* ctx, const uint8_t* sigs, const mbls_msgtable* mt, const uint32_t* msg_idx, const uint8_t* pks, int pk_format, uint64_t n,
                               uint8_t* results, uint32_t* status);
int mbls_fast_aggregate_verify_batch_indexed_msgtable_device(mbls_ctx* ctx, const mbls_keytable* t, const uint8_t* d_sigs, const mbls_msgtable* mt,
                                                             const uint32_t* d_msg_idx, const uint32_t* d_key_idx, const uint32_t* d_offsets, uint64_t n, uint32_t k,
                                                             uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream);
int mbls_fast_aggregate_verify_batch_indexed_msgtable(mbls_ctx* ctx, const mbls_keytable* t, const uint8_t* sigs, const mbls_msgtable* mt, const uint32_t* msg_idx,
                                                      const uint32_t* key_idx, const uint32_t* offsets, uint64_t n, uint32_t k, uint8_t* results, uint32_t* status);

/* ---- committee table: fast_aggregate_verify by participation bits -------------------------------------------
 * An Ethereum aggregate names a COMMITTEE -- an ordered member list fixed for an epoch -- and a bitfield of who signed, and nearly everyone signs. The _indexed
 * entries make the caller expand every bitfield into uint32 indices (512 bytes per item of a 128-member committee instead of 16) and add 127 keys where one
 * subtraction would do. A committee table lives on the key side, bound to ONE key table of the same context: committee `id` is an ordered list of key-table
 * indices, kept in HBM with its full key sum (what the beacon state stores as the sync committee's aggregate_pubkey) and an ELIGIBLE flag, set only if every
 * member is a valid, finite table entry. A verification item names a committee and carries a bitfield; on the device each item takes one of two routes:
 *   direct:      the sum of the members whose bit is set (s additions),
 *   complement:  the cached full sum minus the sum of the members whose bit is clear ((m - s) additions and one fix-up addition).
 * Complement is taken only for an eligible committee -- only there are the MBLS_ST_BAD_PK_ENCODING / MBLS_ST_PK_INFINITY bits of every subset known to be zero,
 * so the status word does not depend on the route -- and, in the automatic mode, when (m - s) + 1 < s: a count of additions, not a measurement.
 * TABLE. mbls_committees_create binds the table to `keytable` (capacity_hint committees, 0: 64; growth keeps every id and drains the device, like the key
 *   table's). Destroy a committee table before its key table: mbls_keytable_destroy unbinds the committee tables still bound to it, which then refuse appends
 *   and verifications with MBLS_ERR_ARGUMENT and accept count, get, clear and destroy. A table whose context went first is an empty shell that only
 *   mbls_committees_destroy accepts (mbls_committees_count is 0). Ids start at 0 and are stable until mbls_committees_clear.
 * APPEND (host memory; a device-pointer append is out of scope). Committee first_id + c has members key_idx[offsets[c] .. offsets[c+1]), in that order; bit j of an
 *   item's bitfield means member j. MBLS_ERR_ARGUMENT, and nothing appended, for: an offset table that runs backwards, an empty committee, a committee of more than
 *   MBLS_COMMITTEE_MAX_MEMBERS members (the protocol's limit), an index at or above the key table's size at the time of the call. Duplicated members are allowed.
 *   The member lists are stored on the device, the full sums are computed there by the indexed key-sum routine (in the context's workspace, ordered against its
 *   other users) and k_cmt_build turns them into records. ORDERING is mbls_keytable_append_device's: the append waits on the device for pending appends to the key
 *   table, and verifications on any stream wait on the device for the append. n_committees = 0 is MBLS_OK with *first_id = count.
 * mbls_committees_get returns the cached sum as 96 uncompressed bytes (AggregatePublicKey::aggregate over the members, reference src/aggregates.rs:29-39; the
 *   point at infinity in the reference's encoding), the member count and the eligible flag. Any of the three outputs may be NULL.
 * mbls_committees_clear BLOCKS until every append and verification enqueued over the table has finished (it drains the device, like mbls_msgtable_clear), then
 *   sets the count to 0 and keeps the capacity: the next append starts at id 0. The intended use is one clear per epoch boundary.
 * VERIFICATION ENTRIES. The arguments of the _indexed / _indexed_msgtable entries with `key_idx, offsets, k` replaced by `committees, cmt_idx, bits, bits_stride`
 *   (the key table is the one the committee table is bound to): item i uses committee cmt_idx[i] and the bits_stride bytes at bits + bits_stride * i; member j is
 *   selected when (byte[j >> 3] >> (j & 7)) & 1 -- SSZ bit order, so a Bitvector or a Bitlist is passed as serialized. Bits at positions at or above the
 *   committee's size are IGNORED: a Bitlist's delimiter bit may stay, and checking the Bitlist's length against the committee remains the caller's job.
 *   bits_stride is a multiple of 4 and 8 * bits_stride covers the largest committee the table holds; d_bits of the device entries is 4-byte aligned (the host
 *   entries stage the bytes and accept any alignment). Otherwise MBLS_ERR_ARGUMENT.
 *   results[i], the bitmap and status[i] are bit for bit what mbls_fast_aggregate_verify_batch_indexed[_msgtable] returns for the same signatures and messages with
 *   the selected members spelled out in member order through a ragged offset table -- on either route, under every routing mode: no bit set gives MBLS_ST_NO_KEYS,
 *   a selected sum at infinity MBLS_ST_APK_INFINITY. The table is read at the count it has when the call is enqueued. DEVICE entries reject an item whose
 *   cmt_idx[i] is at or above that count like an index outside the key table (MBLS_ST_BAD_PK_ENCODING among its bits, result 0: exactly the words of an item that
 *   lists the one key index 0xFFFFFFFF); HOST entries refuse the call with MBLS_ERR_ARGUMENT before anything is enqueued. n = 0 is MBLS_OK with nothing written.
 *   Routing of the batch is mbls_plan_batch(limits, n), workspace mbls_plan_workspace_items(limits, n, 0, 0) (the committee form never takes the eight-lane key
 *   split: it is ragged, and complement lists are short).
 * ALLOCATION. k_cmt_expand writes every item's index list into a scratch of the context: items x (largest committee) uint32, plus two words per item. A call
 *   reserves it before it queues the first pass of its plan (growth drains the device, see mbls_ctx_reserve); mbls_ctx_reserve_committee_items(ctx, max_items,
 *   max_members) beforehand keeps the allocation out of the call.
 * ROUTE (mbls_ctx_set_committee_route; mbls_ctx_reset_tuning restores 0): 0 auto, 1 always direct, 2 complement whenever the committee is eligible.
 *   mbls_plan_committee_route(m, s, eligible, mode) states the decision without a GPU -- the SAME function the kernel runs (csrc/mbls_cmt.h): 1 complement,
 *   0 direct, MBLS_ERR_ARGUMENT for a mode outside 0..2, m = 0, m > MBLS_COMMITTEE_MAX_MEMBERS or s > m.
 * OUT OF SCOPE: the shared-list message form, the mbls_multi handle, a device-pointer append. (verify_multiple over committees:
 * mbls_verify_multiple_committee_msgtable*, below; the verification stream over committees: mbls_stream_create_committee, below.) */
#define MBLS_COMMITTEE_MAX_MEMBERS 2048
typedef struct mbls_committees mbls_committees;
int mbls_committees_create(mbls_ctx* ctx, mbls_keytable* keytable, uint64_t capacity_hint, mbls_committees** out);
void mbls_committees_destroy(mbls_committees* t);
uint64_t mbls_committees_count(const mbls_committees* t);
uint32_t mbls_committees_max_members(const mbls_committees* t);     /* the largest committee the table holds (0: none): what 8 * bits_stride has to cover */
int mbls_committees_clear(mbls_committees* t);
int mbls_committees_append(mbls_committees* t, const uint32_t* key_idx, const uint32_t* offsets, uint64_t n_committees, uint64_t* first_id);
int mbls_committees_get(mbls_committees* t, uint64_t id, uint8_t* sum96, uint32_t* n_members, uint32_t* eligible);
int mbls_ctx_set_committee_route(mbls_ctx* ctx, int mode);
int mbls_plan_committee_route(uint32_t m, uint32_t s, int eligible, int mode);
int mbls_ctx_reserve_committee_items(mbls_ctx* ctx, uint64_t max_items, uint32_t max_members);
int mbls_fast_aggregate_verify_batch_committee_device(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* d_sigs, const uint8_t* d_msgs,
                                                      uint32_t msg_len, const uint64_t* d_msg_offsets, const uint32_t* d_cmt_idx, const uint8_t* d_bits,
                                                      uint32_t bits_stride, uint64_t n, uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream);
int mbls_fast_aggregate_verify_batch_committee(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len,
                                               const uint64_t* msg_offsets, const uint32_t* cmt_idx, const uint8_t* bits, uint32_t bits_stride, uint64_t n,
                                               uint8_t* results, uint32_t* status);
int mbls_fast_aggregate_verify_batch_committee_msgtable_device(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* d_sigs, const mbls_msgtable* mt,
                                                               const uint32_t* d_msg_idx, const uint32_t* d_cmt_idx, const uint8_t* d_bits, uint32_t bits_stride,
                                                               uint64_t n, uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream);
int mbls_fast_aggregate_verify_batch_committee_msgtable(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* sigs, const mbls_msgtable* mt,
                                                        const uint32_t* msg_idx, const uint32_t* cmt_idx, const uint8_t* bits, uint32_t bits_stride, uint64_t n,
                                                        uint8_t* results, uint32_t* status);

/* ---- committee spans: fast_aggregate_verify over several committees per item -------------------------------
 * Since Electra (EIP-7549) an on-chain attestation names up to 64 committees of its slot (committee_bits) and carries ONE bitfield, the concatenation of those
 * committees' participation bits (aggregation_bits), under one signature over one signing root. The committee entries above serve one committee per item; these
 * entries serve the span, without the caller expanding the field into uint32 indices (about 128 KB per item at mainnet sizes against 4 KB of bits) and without
 * the device adding every one of those keys.
 * ITEM. Item i names the committees c_0 .. c_(q-1) = cmt_ids[cmt_off[i] .. cmt_off[i + 1]) of `committees` -- cmt_off holds n + 1 ABSOLUTE offsets into the
 *   n_cmt_ids ids, like the offsets of a ragged key table --, q <= MBLS_SPAN_MAX_COMMITTEES; an id may appear more than once. With m_t the size of c_t,
 *   o_t = m_0 + ... + m_(t-1) and M = o_q, member j of c_t is selected when bit o_t + j of the bits_stride bytes at bits + bits_stride * i is set (SSZ bit order,
 *   as above). Bits at or above M are IGNORED: a Bitlist's delimiter may stay. 8 * bits_stride >= M is required of every item; bits_stride is a multiple of 4, and
 *   d_bits of the device entries is 4-byte aligned.
 * KEY SUM. Every segment takes its own route, from the SAME function as the committee entries (csrc/mbls_cmt.h cmt_route(m_t, s_t, eligible_t, mode), under
 *   mbls_ctx_set_committee_route). The item's key sum is the sum of the selected members of its direct segments plus, for every complement segment, the cached
 *   sum of c_t minus the sum of its missing members.
 *   results[i], the bitmap and status[i] are bit for bit what mbls_fast_aggregate_verify_batch_indexed[_msgtable] returns for the same signature and message with
 *   the selected members spelled out in (segment, member) order -- on every mix of routes, under all three route modes: MBLS_ST_NO_KEYS exactly when no member of
 *   the whole item is selected (q = 0 included), MBLS_ST_APK_INFINITY from the final point, MBLS_ST_PK_INFINITY / MBLS_ST_BAD_PK_ENCODING only as the direct
 *   segments of ineligible committees produce them. A span of one committee returns exactly the _committee[_msgtable] entry's outputs.
 * MALFORMED ITEMS: an id at or above the table's count, q > 64, cmt_off[i + 1] < cmt_off[i], cmt_off[i + 1] > n_cmt_ids, or M > 8 * bits_stride. DEVICE entries
 *   reject such an item like an item that lists the one key index 0xFFFFFFFF (the committee entries' convention, the same words: MBLS_ST_BAD_PK_ENCODING among its
 *   bits, result 0), and read nothing outside cmt_ids, the item's field or the table: the offsets are checked before the ids, the ids before the records, M before
 *   the field. HOST entries refuse the call with MBLS_ERR_ARGUMENT before anything is enqueued and leave the outputs unwritten. n = 0 is MBLS_OK.
 * ROUTING of the batch is mbls_plan_batch(limits, n), the workspace mbls_plan_workspace_items(limits, n, 0, 0): the span form adds no workspace item.
 * ALLOCATION. k_cms_expand leaves two lists per item -- the selected members of direct segments, the missing members of complement segments -- in one region of
 *   stride = min(8 * bits_stride, 64 * mbls_committees_max_members) uint32 (they never exceed M entries together and grow from its two ends), a record of 5 words
 *   and a parked point of 36 words. A call reserves this for the extent of its plan before it queues anything: 4 * stride + 164 bytes per item of a round. This is
 *   LARGE at mainnet sizes: with bits_stride = 4 096 a full round of 65 536 items takes 8 GiB; size bits_stride to the attestations at hand (64 committees of 128
 *   members need 1 024 bytes: 2 GiB per round) or lower mbls_ctx_set_round_items. An allocation that fails is MBLS_ERR_DEVICE, nothing enqueued.
 *   mbls_ctx_reserve_committee_span_items(ctx, max_items, max_item_members) beforehand keeps the allocation out of the call (max_item_members: the stride, at most
 *   64 * MBLS_COMMITTEE_MAX_MEMBERS). mbls_ctx_reserve_committee_items and its limit are unchanged.
 * mbls_plan_committee_span states, without a GPU, what the kernel decides for one item from the same header functions (csrc/mbls_cms.h): sizes[t] and eligible[t]
 *   of the q segments, the item's field (bits_bytes bytes, any alignment) and the route mode in; the mask of the segments that go complement (bit t: segment t)
 *   and the entries of the direct and of the missing list out. MBLS_ERR_ARGUMENT for q > 64, a size of 0 or above MBLS_COMMITTEE_MAX_MEMBERS, M > 8 * bits_bytes,
 *   a mode outside 0..2 or a null output.
 * OUT OF SCOPE: the verification stream, the shared-list message form, the mbls_multi handle. (verify_multiple over spans:
 * mbls_verify_multiple_committee_span_msgtable* below.) */
#define MBLS_SPAN_MAX_COMMITTEES 64
int mbls_fast_aggregate_verify_batch_committee_span_device(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* d_sigs, const uint8_t* d_msgs,
                                                           uint32_t msg_len, const uint64_t* d_msg_offsets, const uint32_t* d_cmt_ids, uint64_t n_cmt_ids,
                                                           const uint32_t* d_cmt_off, const uint8_t* d_bits, uint32_t bits_stride, uint64_t n, uint8_t* d_results,
                                                           uint64_t* d_bitmap, uint32_t* d_status, void* stream);
int mbls_fast_aggregate_verify_batch_committee_span(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len,
                                                    const uint64_t* msg_offsets, const uint32_t* cmt_ids, uint64_t n_cmt_ids, const uint32_t* cmt_off,
                                                    const uint8_t* bits, uint32_t bits_stride, uint64_t n, uint8_t* results, uint32_t* status);
int mbls_fast_aggregate_verify_batch_committee_span_msgtable_device(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* d_sigs, const mbls_msgtable* mt,
                                                                    const uint32_t* d_msg_idx, const uint32_t* d_cmt_ids, uint64_t n_cmt_ids,
                                                                    const uint32_t* d_cmt_off, const uint8_t* d_bits, uint32_t bits_stride, uint64_t n,
                                                                    uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream);
int mbls_fast_aggregate_verify_batch_committee_span_msgtable(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* sigs, const mbls_msgtable* mt,
                                                             const uint32_t* msg_idx, const uint32_t* cmt_ids, uint64_t n_cmt_ids, const uint32_t* cmt_off,
                                                             const uint8_t* bits, uint32_t bits_stride, uint64_t n, uint8_t* results, uint32_t* status);
int mbls_ctx_reserve_committee_span_items(mbls_ctx* ctx, uint64_t max_items, uint32_t max_item_members);
int mbls_plan_committee_span(const uint32_t* sizes, const uint8_t* eligible, uint32_t q, const uint8_t* bits, uint32_t bits_bytes, int mode,
                             uint64_t* complement_mask, uint32_t* n_direct_listed, uint32_t* n_missing_listed);

/* ---- verification stream: many small calls packed into full rounds ---------------------------------------
 * The verification entries run at their full rate only when one call carries a whole round (CUs x 4 x 64 items, 65 536 on MI355X). A
 * stream takes calls of ANY size, hands back a ticket per call, packs the items of many calls back to back into full-round launches of
 * the entries above, and puts each call's results back where that call asked for them.
 * STREAM. Belongs to one context; fixed at creation to one mode (MBLS_STREAM_FAST_AGGREGATE_VERIFY: reference src/aggregates.rs:177-215,
 *   MBLS_STREAM_VERIFY: src/signature.rs:27-40) and one key source: pk_format MBLS_PK_UNCOMPRESSED (96-byte keys), MBLS_PK_COMPRESSED
 *   (48-byte keys), or t != NULL: indices into a key table of the same context (fast_aggregate_verify mode only).
 * CALLS. Each call has the shape of a mbls_fast_aggregate_verify_batch[_indexed]_device / mbls_verify_batch_device call: n >= 1 items,
 *   messages msg_len bytes each or ragged through h_msg_offsets, keys k per item or ragged through h_pk_offsets (verify mode: k = 1 and no
 *   key offsets), per-item results, optional status words and (device submits) an optional packed bitmap. Results, status words and bitmap
 *   are bit-identical to what that direct entry returns for the same inputs, every MBLS_ST_* bit included.
 * OFFSET TABLES LIVE IN HOST MEMORY for both submit entries, even when the bytes they index are on the device: the library cuts rounds
 *   with them. At submit they are checked as the host entries check theirs (non-decreasing, messages below 2^32 bytes); a bad table
 *   refuses the call with MBLS_ERR_ARGUMENT and the call gets no ticket.
 * PACKING. Items are packed densely, in submission order, into rounds of round_items items (default: the context's round,
 *   mbls_ctx_get_limits), round_keys keys (default 128 x round_items) and round_msg_bytes message bytes (default 64 x round_items); the
 *   stream's staging buffers are sized from these. A round closes when it is full or when the next item's keys or message would not fit;
 *   a call may be split across rounds. An item that does not fit an empty round is refused at submit (MBLS_ERR_ARGUMENT, the message
 *   names the capacity).
 * LAUNCH. A round always launches when it is full, on mbls_stream_flush, on mbls_stream_wait for a call in it, and on destroy. Policy
 *   MBLS_STREAM_WORK_CONSERVING (default): also as soon as fewer than `depth` launched rounds are unfinished (default 2: one running, one
 *   queued behind it) -- a lone call starts at once, and under load the open round fills while the device is busy. MBLS_STREAM_FULL_ROUNDS:
 *   only full rounds (and flush / wait / destroy): deterministic launches, what tests and throughput runs want.
 * COMPLETION. Rounds finish in order, so calls complete in ticket order: wait(t) = "every ticket <= t is done". mbls_stream_wait blocks
 *   without spinning and returns MBLS_OK or the error of a round that held a piece of the call; mbls_stream_query returns MBLS_PENDING
 *   while the call is not done. An unknown ticket is MBLS_ERR_ARGUMENT. After a device error the stream refuses submits (MBLS_ERR_DEVICE).
 * LIFETIMES AND ORDERING. A device submit records an event on the caller's `stream` (and zeroes the call's bitmap words there first): the
 *   gather of the call's round waits for it, so inputs produced on that stream are safe. The caller's input and output buffers -- host
 *   submits included: their inputs are not copied at submit -- must stay valid and unchanged until the call completes; host results are
 *   in the caller's buffers when wait / query report the call done. Destroy streams before their context.
 * KEY TABLE. Read at the size it has when the call's round launches (entries are never removed: an index valid at submit stays valid).
 * THREADS. Submit, flush, wait, query and stats are thread-safe; any number of threads may share a stream.
 * ALLOCATION. Everything is allocated at creation: the staging slots (depth + 1), the context's workspace for every round size
 *   (mbls_plan_workspace_items) and, for 48-byte keys, the staging of decompressed keys (mbls_ctx_reserve_keys) -- no round grows the
 *   workspace, and the stream never allocates on the device afterwards. */
#define MBLS_PENDING 102
enum { MBLS_STREAM_FAST_AGGREGATE_VERIFY = 0, MBLS_STREAM_VERIFY = 1 };
enum { MBLS_STREAM_WORK_CONSERVING = 0, MBLS_STREAM_FULL_ROUNDS = 1 };
typedef struct mbls_stream mbls_stream;
typedef struct mbls_stream_opts { uint64_t round_items, round_keys, round_msg_bytes; uint32_t depth, policy; } mbls_stream_opts;   /* 0 = default */
/* rounds: launched; full_rounds: of them closed because the next item did not fit; pieces: (call, round) parts; split_calls: calls of
   more than one piece; gathered_bytes: input bytes staged into the rounds */
typedef struct mbls_stream_stats { uint64_t calls, items, pieces, rounds, full_rounds, split_calls, gathered_bytes; } mbls_stream_stats;
/* opts may be NULL (every default); t != NULL makes an index stream (pk_format is then ignored) */
int mbls_stream_create(mbls_ctx* ctx, int mode, int pk_format, const mbls_keytable* t, const mbls_stream_opts* opts, mbls_stream** out);
void mbls_stream_destroy(mbls_stream* s);                /* flushes, waits for every call, frees */
const char* mbls_stream_last_error(mbls_stream* s);
/* device buffers, host offset tables; d_pks for byte-key streams, d_key_idx for index streams (the other NULL) */
int mbls_stream_submit_device(mbls_stream* s, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* h_msg_offsets,
                              const uint8_t* d_pks, const uint32_t* d_key_idx, const uint32_t* h_pk_offsets, uint64_t n, uint32_t k,
                              uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream, uint64_t* ticket);
/* host buffers (read when the call's round launches, written when it completes) */
int mbls_stream_submit(mbls_stream* s, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* msg_offsets,
                       const uint8_t* pks, const uint32_t* key_idx, const uint32_t* pk_offsets, uint64_t n, uint32_t k,
                       uint8_t* results, uint32_t* status, uint64_t* ticket);
/* A stream over a resident message table (see "resident message table"): same modes, key sources, policies, depth, threading, completion order and lifetime
 * rules; a call names its messages by table index. A round stages 4 bytes per item where it staged the message -- the index array is the "message bytes" of a
 * call shape with msg_len = 4 and no offsets, so rounds are cut exactly as mbls_stream_cut cuts calls of msg_len = 4, and round_msg_bytes defaults to
 * 4 x round_items -- and launches the `_msgtable_device` entry of its mode. The table is read at the size it has when the call's round launches (the key table's
 * rule; mbls_msgtable_clear is refused while calls are pending, so an index valid at submit stays valid); in both submit forms an index at or above that size
 * rejects its item with MBLS_ST_BAD_MSG_RANGE, as an out-of-range key index rejects its item. Per-call results, status words and bitmap are byte for byte what a
 * direct `_msgtable_device` call on the same inputs returns. mbls_stream_submit[_device] on such a stream, and the two entries below on a stream of
 * mbls_stream_create, are MBLS_ERR_ARGUMENT. */
int mbls_stream_create_msgtable(mbls_ctx* ctx, int mode, int pk_format, const mbls_keytable* t, mbls_msgtable* mt, const mbls_stream_opts* opts, mbls_stream** out);
int mbls_stream_submit_msgidx_device(mbls_stream* s, const uint8_t* d_sigs, const uint32_t* d_msg_idx, const uint8_t* d_pks, const uint32_t* d_key_idx,
                                     const uint32_t* h_pk_offsets, uint64_t n, uint32_t k, uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream,
                                     uint64_t* ticket);
int mbls_stream_submit_msgidx(mbls_stream* s, const uint8_t* sigs, const uint32_t* msg_idx, const uint8_t* pks, const uint32_t* key_idx, const uint32_t* pk_offsets,
                              uint64_t n, uint32_t k, uint8_t* results, uint32_t* status, uint64_t* ticket);
/* A stream over a committee table and a message table (see "committee table"): the smallest item -- a committee id, a participation bitfield as SSZ serializes
 * it, a message-table index -- for the caller with the smallest calls. Mode fast_aggregate_verify only. The stream is bound to ONE committee table, through it to
 * that table's key table, and to ONE message table, all of the stream's context; policies, depth, threading, ticket order, flush / wait / query, lifetimes and
 * mbls_stream_get_stats are the stream's above, unchanged.
 * CREATE. bits_stride is fixed at creation: a multiple of 4 with 8 * bits_stride >= mbls_committees_max_members(committees) at that moment. MBLS_ERR_ARGUMENT for a
 *   null table, a committee table whose key table is gone, tables of another context, a stride that is not a multiple of 4 or does not cover the largest committee.
 * CALL. n >= 1 items; item i has its 96-byte signature, msg_idx[i], cmt_idx[i] and the bits_len bytes at bits + bits_len * i. bits_len is a value of the CALL, any
 *   number in 1 .. bits_stride -- not necessarily a multiple of 4, and d_bits of a device submit needs no alignment: calls of different producers carry fields of
 *   different lengths (a Bitlist of a 127-member committee is 16 bytes, of a 128-member one 17), and the gather of a round re-strides them on the device
 *   (k_stream_gather_cmt). bits_len = 0 or above the stride is MBLS_ERR_ARGUMENT at submit, and the call gets no ticket.
 * RESULT. Per-call results, status words and bitmap are byte for byte what mbls_fast_aggregate_verify_batch_committee_msgtable_device returns on the same
 *   signatures, indices and ids with every field ZERO-EXTENDED to bits_stride bytes -- every MBLS_ST_* bit, under every mbls_ctx_set_committee_route mode, on every
 *   engine. A field shorter than its committee therefore selects nobody beyond its last byte. BOTH submit forms reject on the device as that entry does -- an id at
 *   or above the table's count like a key index outside the key table, a message index at or above the message table's size with MBLS_ST_BAD_MSG_RANGE --; they do
 *   not refuse the call.
 * CUTTING. A committee call is the shape {n, k = 0, msg_len = 4}: rounds are cut exactly as mbls_stream_cut cuts such shapes; round_msg_bytes defaults to
 *   4 x round_items, round_keys plays no part.
 * ALLOCATION. Everything at creation: a slot holds 96 + 4 + 4 + bits_stride bytes per item (and as many pinned bytes per item as the stride, through which the
 *   fields of host submits are zero-extended); the context's workspace for every round size, and its committee scratch as
 *   mbls_ctx_reserve_committee_items(ctx, round_items, min(8 * bits_stride, MBLS_COMMITTEE_MAX_MEMBERS)). No round allocates. A slot never shows a round the bits
 *   of the round before: every byte of every item's stride is written. mbls_stream_stats.gathered_bytes counts 96 + 4 + 4 + bits_len per item.
 * TABLES. Both are read at the size they have when the call's round launches. While calls of the stream are pending mbls_committees_clear (and
 *   mbls_msgtable_clear) are refused with MBLS_ERR_ARGUMENT, so an id valid at submit stays valid. While the stream lives, mbls_committees_append refuses a committee
 *   of more than 8 * bits_stride members (the smallest stride among the table's streams; MBLS_ERR_ARGUMENT, nothing appended, the message names the stride): such a
 *   committee would make every later round fail the entry's argument check. Destroying the stream releases both interlocks. DESTROY A STREAM BEFORE ITS TABLES.
 * mbls_stream_submit[_device] and mbls_stream_submit_msgidx[_device] on such a stream, and the two entries below on any other stream, are MBLS_ERR_ARGUMENT; the
 *   message names the right entry.
 * OUT OF SCOPE: committee spans in a stream, per-item message bytes or a shared message list in a committee stream, the mbls_multi handle. (verify_multiple in a
 *   stream: mbls_stream_create_vm_committee, below.) */
int mbls_stream_create_committee(mbls_ctx* ctx, mbls_committees* committees, mbls_msgtable* mt, uint32_t bits_stride, const mbls_stream_opts* opts, mbls_stream** out);
int mbls_stream_submit_committee_device(mbls_stream* s, const uint8_t* d_sigs, const uint32_t* d_msg_idx, const uint32_t* d_cmt_idx, const uint8_t* d_bits,
                                        uint32_t bits_len, uint64_t n, uint8_t* d_results, uint64_t* d_bitmap, uint32_t* d_status, void* stream, uint64_t* ticket);
int mbls_stream_submit_committee(mbls_stream* s, const uint8_t* sigs, const uint32_t* msg_idx, const uint32_t* cmt_idx, const uint8_t* bits, uint32_t bits_len,
                                 uint64_t n, uint8_t* results, uint32_t* status, uint64_t* ticket);
int mbls_stream_flush(mbls_stream* s);
int mbls_stream_wait(mbls_stream* s, uint64_t ticket);
int mbls_stream_query(mbls_stream* s, uint64_t ticket);
int mbls_stream_get_stats(mbls_stream* s, mbls_stream_stats* out);
/* Pure (no GPU, no context): how a sequence of calls is cut into rounds -- the same incremental rule the stream's launcher runs -- with a
 * forced launch after call i where flush_after[i] != 0 (opts fully given: no zero defaults). out may be NULL with max_pieces = 0 to count;
 * *n_pieces receives the count. MBLS_ERR_ARGUMENT for null pointers, zero options, no calls, a call of n = 0, a bad offset table, an item
 * larger than an empty round, or more pieces than max_pieces. */
typedef struct mbls_stream_call_shape { uint64_t n; uint32_t k, msg_len; const uint32_t* pk_offsets; const uint64_t* msg_offsets; uint32_t flush_after; } mbls_stream_call_shape;
typedef struct mbls_stream_piece { uint64_t call, first, items, round, round_first; } mbls_stream_piece;
int mbls_stream_cut(const mbls_stream_opts* opts, const mbls_stream_call_shape* calls, uint64_t n_calls,
                    mbls_stream_piece* out, uint64_t max_pieces, uint64_t* n_pieces);
/* A verify_multiple stream over a committee table and a message table: the gossip caller, many threads each holding ONE small verify_multiple batch. A CALL IS A
 * BATCH; a ROUND is one call of mbls_verify_multiple_batches_committee_msgtable_locate_device (below, "MANY verify_multiple BATCHES PER CALL") over the round's
 * slot, with a ragged batch table the launcher builds on the host. Binding to the tables, policies, depth, threading, ticket order, flush / wait / query, lifetimes
 * and mbls_stream_get_stats are the committee stream's above, unchanged; create refuses what mbls_stream_create_committee refuses.
 * CALL. n_sets >= 1 sets, those of mbls_verify_multiple_committee_msgtable_locate_device: set i is cmt_idx[i] (a committee id, or MBLS_VM_SET_SINGLE_KEY | key
 *   index), the bits_len bytes at bits + bits_len * i, msg_idx[i] and the scalar rands[i]. bits_len is a value of the CALL, 0 .. bits_stride, at any alignment;
 *   bits_len = 0 allows bits = NULL (every field is zero: a batch of single-key sets only). The scalars come from the caller, as in every _device entry: NULL is
 *   MBLS_ERR_ARGUMENT, a zero scalar rejects its call with MBLS_ST_BAD_SCALAR. Outputs: one byte (required) and one optional status word per CALL, n_sets bytes and
 *   n_sets optional words per SET (both set arrays may be NULL). n_sets = 0 is MBLS_ERR_ARGUMENT and the call gets no ticket.
 * RESULT. Every output of a call is byte for byte what mbls_verify_multiple_batches_committee_msgtable_locate_device writes for that call alone as one batch
 *   (n_batches = 1, sets_per_batch = n_sets) on the same signatures, ids, indices and scalars with every field ZERO-EXTENDED to bits_stride -- under every mode of
 *   mbls_ctx_set_vm_grouping and mbls_ctx_set_committee_route, however the stream packed the round. No output of a call depends on any other call of its round.
 *   BOTH submit forms reject on the device as that entry does (an id, key index or message index that names nothing); the stream does not refuse the call.
 * CUTTING. A call is never split (a batch's verdict is one pairing product). It costs n_sets + 1 of round_items -- its sets plus its signature pair, so the
 *   per-set route's Miller launch stays within a round --, a call that does not fit the open round closes it, and a call with n_sets + 1 > round_items is refused at
 *   submit (MBLS_ERR_ARGUMENT, the message names the capacity). round_keys and round_msg_bytes play no part. stats.pieces == stats.calls, split_calls == 0,
 *   stats.items counts sets, gathered_bytes counts 96 + 4 + 4 + 8 + bits_len per set. mbls_stream_cut_vm is the rule as data (pure, no GPU): call j of
 *   call_sets[j] sets is piece j = {j, 0, call_sets[j], its round, its first set in the round}, with a forced launch after call j where flush_after[j] != 0
 *   (flush_after may be NULL); only opts->round_items is read. MBLS_ERR_ARGUMENT for null pointers, round_items = 0, no calls, a call of 0 sets or of more than
 *   round_items - 1, or more pieces than max_pieces (out = NULL with max_pieces = 0 counts).
 * max_groups of a round is the sum over its calls of: the exact count of distinct message indices the call names (host submits, counted at submit; n_sets for a
 *   call of more than MBLS_VBG_MAX_SETS sets, which is not grouped), and n_sets for device submits -- the host cannot see their indices, and a wrong promise by one
 *   caller would reject innocent calls behind it in the group space. A per-call hint for device submits is OUT OF SCOPE.
 * ALLOCATION. Everything at creation: a slot holds 96 + 4 + 4 + 8 + bits_stride bytes per set (and as many pinned bytes per set, the mirrors through which host
 *   submits are staged: every run of neighbouring host calls goes up in one copy per array); the context's workspace for every (n_sets, n_batches) a round can
 *   hold on both routes with locate (mbls_plan_verify_multiple_batches_committee), the committee scratch as a committee stream reserves it, and the entry's own
 *   staging (set map, group arrays). No round allocates. A slot never shows a round the bits or scalars of the round before.
 * TABLES. The committee stream's interlocks: mbls_committees_clear and mbls_msgtable_clear are refused while calls are pending, mbls_committees_append refuses a
 *   committee of more than 8 * bits_stride members while the stream lives. DESTROY A STREAM BEFORE ITS TABLES.
 * The other submit entries on such a stream, and the two below on any other stream, are MBLS_ERR_ARGUMENT; the message names the right entry.
 * OUT OF SCOPE: spans in a stream, per-set message bytes or a shared message list, a group-count promise for device submits, the mbls_multi handle, wire keys. */
int mbls_stream_create_vm_committee(mbls_ctx* ctx, mbls_committees* committees, mbls_msgtable* mt, uint32_t bits_stride, const mbls_stream_opts* opts,
                                    mbls_stream** out);
int mbls_stream_submit_vm_device(mbls_stream* s, const uint8_t* d_sigs96, const uint32_t* d_cmt_idx, const uint8_t* d_bits, uint32_t bits_len,
                                 const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n_sets, uint8_t* d_result, uint32_t* d_status, uint8_t* d_set_results,
                                 uint32_t* d_set_status, void* stream, uint64_t* ticket);
int mbls_stream_submit_vm(mbls_stream* s, const uint8_t* sigs96, const uint32_t* cmt_idx, const uint8_t* bits, uint32_t bits_len, const uint32_t* msg_idx,
                          const uint64_t* rands, uint64_t n_sets, uint8_t* result, uint32_t* status, uint8_t* set_results, uint32_t* set_status, uint64_t* ticket);
int mbls_stream_cut_vm(const mbls_stream_opts* opts, const uint64_t* call_sets, const uint32_t* flush_after, uint64_t n_calls,
                       mbls_stream_piece* out, uint64_t max_pieces, uint64_t* n_pieces);

/* ---- several GPUs behind one handle ------------------------------------------------------------------------
 * Items are independent (reference src/aggregates.rs:177-215 keeps no state between calls), so a batch shards embarrassingly:
 * device g of G verifies items [n g / G, n (g + 1) / G). One context and one host thread per listed device; every thread stages its
 * own shard from the caller's buffers and writes its results into them in place (in a one-process-per-GPU deployment -- bench.py --
 * the same partition is milagro_bls_amd/shard.py and the accept bitmap is gathered with RCCL through torch.distributed).
 * THE EXCHANGE STEPS of the handle -- the packed accept bitmap of mbls_multi_fast_aggregate_verify_bitmap, the partial records of
 * mbls_multi_verify_multiple_aggregate_signatures -- are RCCL all-gathers between the devices' buffers (over xGMI on an MI355X node): the
 * handle opens librccl.so.1 at run time (no link-time dependency) and makes one communicator over its devices (ncclCommInitAll). Where
 * that is not possible -- RCCL absent, the same device listed twice (RCCL wants one rank per device), MBLS_MULTI_NO_RCCL set -- the same
 * records travel through host memory instead: same results, never a restart; mbls_multi_rccl_active / mbls_multi_exchange_note tell which.
 * A device id may be listed more than once (two contexts then share that GPU). Calls on one handle are serialised. */
typedef struct mbls_multi mbls_multi;
int mbls_multi_create(mbls_multi** out, const int* device_ids, int n_devices);
void mbls_multi_destroy(mbls_multi* m);
int mbls_multi_device_count(const mbls_multi* m);
const char* mbls_multi_last_error(mbls_multi* m);
mbls_ctx* mbls_multi_context(mbls_multi* m, int i);            /* the i-th device's context (for the scalar API, reserve, ...) */
int mbls_multi_reserve(mbls_multi* m, uint64_t max_items);     /* workspace for batches of up to max_items items in total */
int mbls_multi_rccl_active(const mbls_multi* m);               /* 1: exchange steps are RCCL all-gathers between the devices; 0: through host memory */
const char* mbls_multi_exchange_note(mbls_multi* m);           /* which, and why (e.g. "host join: device 0 is listed more than once ...") */
/* same arguments, results and status words as mbls_fast_aggregate_verify_batch / mbls_verify_batch (host buffers) */
int mbls_multi_fast_aggregate_verify_batch(mbls_multi* m, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len,
                                           const uint64_t* msg_offsets, const uint8_t* pks, int pk_format, const uint32_t* pk_offsets,
                                           uint64_t n, uint32_t k, uint8_t* results, uint32_t* status);
int mbls_multi_verify_batch(mbls_multi* m, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len, const uint64_t* msg_offsets,
                            const uint8_t* pks, int pk_format, uint64_t n, uint8_t* results, uint32_t* status);
/* n x fast_aggregate_verify with the results as ONE packed accept bitmap that EVERY device of the handle ends up holding (bit i % 64 of word i / 64 =
 * item i): device g verifies the items of words [g W, (g + 1) W), W = ceil(ceil(n / 64) / G), packs them on the device, and the words are all-gathered
 * between the devices (RCCL when active, see above). `bitmap` (host, ceil(n / 64) words; may be NULL) receives the first device's copy;
 * mbls_multi_device_bitmap(m, g) is device g's own copy (a device pointer to G W words, valid until the next call on the handle). Other arguments
 * as mbls_multi_fast_aggregate_verify_batch. */
int mbls_multi_fast_aggregate_verify_bitmap(mbls_multi* m, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len,
                                            const uint64_t* msg_offsets, const uint8_t* pks, int pk_format, const uint32_t* pk_offsets,
                                            uint64_t n, uint32_t k, uint64_t* bitmap, uint32_t* status);
const uint64_t* mbls_multi_device_bitmap(mbls_multi* m, int g);
/* verify_multiple_aggregate_signatures over the devices of the handle: device g runs sets [n g / G, n (g + 1) / G) up to its partial record
 * (mbls_verify_multiple_partial_device), the G records are all-gathered between the devices (RCCL when active), the first device joins them and
 * runs the tail: the same bool as mbls_verify_multiple_aggregate_signatures on one device, same arguments. */
int mbls_multi_verify_multiple_aggregate_signatures(mbls_multi* m, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs,
                                                    uint32_t msg_len, const uint64_t* msg_offsets, const uint64_t* rands, size_t n);
/* a key table replicated on every device of the handle: same indices everywhere */
typedef struct mbls_multi_keytable mbls_multi_keytable;
int mbls_multi_keytable_create(mbls_multi* m, uint64_t capacity_hint, mbls_multi_keytable** out);
void mbls_multi_keytable_destroy(mbls_multi_keytable* t);
uint64_t mbls_multi_keytable_size(const mbls_multi_keytable* t);
/* All or nothing: when one device fails (or the replicas disagree) the replicas that did append drop the new records again, the
 * indices stay the same on every device and the error names the device (mbls_multi_last_error). */
int mbls_multi_keytable_append(mbls_multi_keytable* t, const uint8_t* pks, int pk_format, int validate, uint64_t n, uint64_t* first_index, uint8_t* errs);
/* replica i of the table (the table of mbls_multi_context(m, i)); owned by the handle */
mbls_keytable* mbls_multi_keytable_replica(mbls_multi_keytable* t, int i);
int mbls_multi_fast_aggregate_verify_batch_indexed(mbls_multi* m, const mbls_multi_keytable* t, const uint8_t* sigs, const uint8_t* msgs,
                                                   uint32_t msg_len, const uint64_t* msg_offsets, const uint32_t* key_idx, const uint32_t* offsets,
                                                   uint64_t n, uint32_t k, uint8_t* results, uint32_t* status);

/* ---- scalar API, 1:1 with the reference's methods (each runs the batch kernels with n = 1) ---- */
/* PublicKey::from_bytes (src/keys.rs:140-147): compressed decode + KeyValidate -> 96-byte decoded key */
int mbls_pk_from_bytes(mbls_ctx* ctx, const uint8_t* bytes, size_t len, uint8_t pk_out[96]);
/* PublicKey::from_bytes_unchecked (src/keys.rs:150-155) */
int mbls_pk_from_bytes_unchecked(mbls_ctx* ctx, const uint8_t* bytes, size_t len, uint8_t pk_out[96]);
/* PublicKey::from_uncompressed_bytes (src/keys.rs:170-175) */
int mbls_pk_from_uncompressed_bytes(mbls_ctx* ctx, const uint8_t* bytes, size_t len, uint8_t pk_out[96]);
/* PublicKey::as_bytes (src/keys.rs:158-160) */
int mbls_pk_as_bytes(mbls_ctx* ctx, const uint8_t pk[96], uint8_t out[48]);
/* PublicKey::key_validate (src/keys.rs:181-186) -> 1/0 */
int mbls_pk_key_validate(mbls_ctx* ctx, const uint8_t pk[96]);
/* PublicKey::from_secret_key (src/keys.rs:124-137); sk range is checked like SecretKey::from_bytes (src/keys.rs:80-82) */
int mbls_pk_from_secret_key(mbls_ctx* ctx, const uint8_t* sk, size_t sk_len, uint8_t pk_out[96]);
/* Signature::from_bytes / AggregateSignature::from_bytes (src/signature.rs:43-46, src/aggregates.rs:319-322) */
int mbls_sig_from_bytes(mbls_ctx* ctx, const uint8_t* bytes, size_t len, uint8_t sig_out[96]);
/* Signature::new (src/signature.rs:17-21) */
int mbls_sign(mbls_ctx* ctx, const uint8_t* msg, size_t msg_len, const uint8_t* sk, size_t sk_len, uint8_t sig_out[96]);
/* Signature::verify (src/signature.rs:27-40) -> 1/0 */
int mbls_verify(mbls_ctx* ctx, const uint8_t sig[96], const uint8_t* msg, size_t msg_len, const uint8_t pk[96]);
/* AggregatePublicKey::aggregate / into_aggregate (src/aggregates.rs:29-56): n decoded keys -> decoded aggregate */
int mbls_aggregate_public_keys(mbls_ctx* ctx, const uint8_t* pks96, size_t n, uint8_t apk_out[96]);
/* AggregatePublicKey::add / add_aggregate (src/aggregates.rs:68-77) */
int mbls_aggregate_public_key_add(mbls_ctx* ctx, const uint8_t a[96], const uint8_t b[96], uint8_t out[96]);
/* AggregateSignature::add / add_aggregate (src/aggregates.rs:114-124); AggregateSignature::new() is 0xC0||0.. */
int mbls_aggregate_signature_add(mbls_ctx* ctx, const uint8_t a[96], const uint8_t b[96], uint8_t out[96]);
/* AggregateSignature::fast_aggregate_verify (src/aggregates.rs:177-215) -> 1/0 */
int mbls_fast_aggregate_verify(mbls_ctx* ctx, const uint8_t sig[96], const uint8_t* msg, size_t msg_len,
                               const uint8_t* pks96, size_t n_pks);
/* AggregateSignature::fast_aggregate_verify_pre_aggregated (src/aggregates.rs:223-253) -> 1/0 */
int mbls_fast_aggregate_verify_pre_aggregated(mbls_ctx* ctx, const uint8_t sig[96], const uint8_t* msg, size_t msg_len,
                                              const uint8_t apk[96]);
/* AggregateSignature::aggregate_verify (src/aggregates.rs:130-170): n messages of msg_lens[i] bytes, concatenated */
int mbls_aggregate_verify(mbls_ctx* ctx, const uint8_t sig[96], const uint8_t* msgs, const size_t* msg_lens, size_t n_msgs,
                          const uint8_t* pks96, size_t n_pks);
/* n x AggregateSignature::aggregate_verify (src/aggregates.rs:130-170) in one call. The (message, key) pairs of all items lie back to back:
 * pair j = (message j, key pks96 + 96 j); messages are msg_len bytes each or msgs[msg_offsets[j] .. msg_offsets[j+1]) (total_pairs + 1
 * offsets); item i owns the pairs [pair_offsets[i], pair_offsets[i+1]) (n + 1 offsets starting at 0) or k each (pair_offsets == NULL) --
 * "as many messages as keys" (src/aggregates.rs:131) holds by construction, an item without pairs is false (MBLS_ST_NO_KEYS). results[i] =
 * 1/0, status[i] = the MBLS_ST_* bits of the item (its signature's and its pairs' ORed). One lane per pair walks the key decode, the
 * message phase and a one-pair Miller loop; the (sig_i, -G1) pairs ride the same launch; a product tree per item; one final exponentiation
 * per item. The device entry only enqueues (total_pairs = pair_offsets[n] must be given: it sizes the launches). */
int mbls_aggregate_verify_batch(mbls_ctx* ctx, const uint8_t* sigs96, const uint8_t* msgs, uint32_t msg_len, const uint64_t* msg_offsets,
                                const uint8_t* pks96, const uint32_t* pair_offsets, uint32_t k, uint64_t n, uint8_t* results, uint32_t* status);
int mbls_aggregate_verify_batch_device(mbls_ctx* ctx, const uint8_t* d_sigs96, const uint8_t* d_msgs, uint32_t msg_len,
                                       const uint64_t* d_msg_offsets, const uint8_t* d_pks96, const uint32_t* d_pair_offsets, uint32_t k,
                                       uint64_t total_pairs, uint64_t n, uint8_t* d_results, uint32_t* d_status, void* stream);
/* AggregateSignature::verify_multiple_aggregate_signatures (src/aggregates.rs:261-316): n sets of
 * (aggregate signature, aggregate public key, message); rands[i] = the NONZERO blinding scalars (63 bits in the
 * reference) drawn from the caller's RNG exactly as at src/aggregates.rs:280-287 -- the reference owns that loop, here
 * the caller does. The scalars are the security of the batch check: rands == NULL is MBLS_ERR_ARGUMENT, and a zero
 * scalar (which would drop its set from the check) makes the check fail: 0 from the bool form; from the *_device forms
 * *d_result = 0 and MBLS_ST_BAD_SCALAR in the status word. One bool for the whole batch.
 * The *_device forms ONLY ENQUEUE (no host synchronisation anywhere): *d_result (one byte of device memory) receives 1 / 0,
 * *d_status (optional, one device word) the OR of the MBLS_ST_* bits of all sets -- a signature outside G2 (the reference's early
 * `return false`, src/aggregates.rs:274-276), an undecodable member or a zero scalar give 0 through it. */
int mbls_verify_multiple_aggregate_signatures(mbls_ctx* ctx, const uint8_t* sigs96, const uint8_t* apks96,
                                              const uint8_t* msgs, uint32_t msg_len, const uint64_t* msg_offsets,
                                              const uint64_t* rands, size_t n);
int mbls_verify_multiple_aggregate_signatures_device(mbls_ctx* ctx, const uint8_t* d_sigs96, const uint8_t* d_apks96,
                                              const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_msg_offsets,
                                              const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status,
                                              void* stream);
/* The reference's own shape, generator included (src/aggregates.rs:261-316): its loop tests set i's signature for the subgroup
 * (:272-275) BEFORE it draws rand[i] from the caller's rng (:280-287) and returns at the first signature outside G2, so a rejected
 * batch leaves the rng after exactly as many draws as sets came before the bad one. This entry keeps that order in ONE call: the
 * signatures are decoded and tested first (beside the message phase), the host reads the verdicts, `draw(user, out, count)` is
 * called at most once for the `count` scalars of the sets in front of the first bad signature (count = n when there is none;
 * not called for count = 0 or n = 0) and must fill out[0 .. count) with NONZERO scalars in set order; what follows does not repeat
 * the subgroup test. Same bool as mbls_verify_multiple_aggregate_signatures with the same scalars. `draw` runs on the calling
 * thread while the context is locked and the call's staging buffers are in use: it must not call back into the library with
 * this context (another context is fine). include/milagro_bls.hpp, rust/src/lib.rs and milagro_bls_amd/api.py draw as :280-287 does. */
typedef void (*mbls_scalar_source)(void* user, uint64_t* out, uint64_t count);
int mbls_verify_multiple_aggregate_signatures_rng(mbls_ctx* ctx, const uint8_t* sigs96, const uint8_t* apks96,
                                              const uint8_t* msgs, uint32_t msg_len, const uint64_t* msg_offsets,
                                              size_t n, mbls_scalar_source draw, void* user);
/* The several-device form (mbls_multi_verify_multiple_aggregate_signatures) with the reference's RNG order and no second subgroup test (what mbls_verify_multiple_aggregate_signatures_rng is to one device): every device decodes and
 * tests its shard's signatures first, the host finds the first bad signature of the WHOLE batch, `draw` is asked ONCE for the scalars of the sets in front of it
 * (reference src/aggregates.rs:272-287) and -- every signature good -- the devices go on from the points they hold to their records, the exchange and the join. */
int mbls_multi_verify_multiple_aggregate_signatures_rng(mbls_multi* m, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs,
                                                        uint32_t msg_len, const uint64_t* msg_offsets, size_t n, mbls_scalar_source draw, void* user);

/* The same for sets given by their keys in wire format (BASELINE configs[3]: 2^14 sets x 128 keys): set i owns k keys
 * (or [pk_offsets[i], pk_offsets[i+1])), AggregatePublicKey::aggregate (src/aggregates.rs:29-39) runs on the device first. */
int mbls_verify_multiple_sets_device(mbls_ctx* ctx, const uint8_t* d_sigs96, const uint8_t* d_pks, int pk_format,
                                     const uint32_t* d_pk_offsets, uint32_t k, const uint8_t* d_msgs, uint32_t msg_len,
                                     const uint64_t* d_msg_offsets, const uint64_t* d_rands, uint64_t n, uint8_t* d_result,
                                     uint32_t* d_status, void* stream);

/* The same for sets named by indices into a resident key table (mbls_keytable_*; the deployment's form: a set is a list of validator indices):
 * set i owns d_key_idx[d_offsets[i] .. d_offsets[i+1]) or k indices each; an index outside the table or an invalid record rejects the check
 * (MBLS_ST_BAD_PK_ENCODING in the status word). With d_partial != NULL the call produces the shard record of the section below instead of
 * d_result / d_status (which may then be NULL). Enqueues only. */
int mbls_verify_multiple_sets_indexed_device(mbls_ctx* ctx, const mbls_keytable* t, const uint8_t* d_sigs96, const uint32_t* d_key_idx,
                                             const uint32_t* d_offsets, uint32_t k, const uint8_t* d_msgs, uint32_t msg_len,
                                             const uint64_t* d_msg_offsets, const uint64_t* d_rands, uint64_t n, uint8_t* d_result,
                                             uint32_t* d_status, uint8_t* d_partial, void* stream);

/* verify_multiple over several devices or processes ("one exchange step"; the reference's function is one loop over
 * one iterator, src/aggregates.rs:261-316 -- the product of pairings and the sum of blinded signatures it accumulates are associative, so
 * the sets may be cut into shards): every participant runs mbls_verify_multiple_partial_device over ITS sets and gets one
 * MBLS_VM_PARTIAL_BYTES record (the shard's Miller product, its sum of [r_i] sig_i, the OR of its status words; opaque, in the library's
 * own number format: exchange it only between builds of the same library); the records are exchanged (RCCL all-gather of G x 896 bytes, or
 * through the host), and mbls_verify_multiple_finish_device joins G records -- any G >= 0, in any order as long as every participant uses
 * the same -- into the bool the one-device call returns for the concatenated sets. Keys: d_apks96 (one aggregate key per set) or, when
 * that is NULL, d_pks / pk_format / d_pk_offsets / k as in mbls_verify_multiple_sets_device. An empty shard (n = 0) is a valid
 * participant. Both entries only enqueue. A record that was not written by mbls_verify_multiple_partial_device -- wrong tag word, or a coefficient
 * of its Miller product that is not below p -- makes the joined check fail (MBLS_ST_PAIRING_FAILED | MBLS_ST_BAD_SIG_ENCODING in the status word). */
#define MBLS_VM_PARTIAL_BYTES 896
int mbls_verify_multiple_partial_device(mbls_ctx* ctx, const uint8_t* d_sigs96, const uint8_t* d_apks96, const uint8_t* d_pks, int pk_format,
                                        const uint32_t* d_pk_offsets, uint32_t k, const uint8_t* d_msgs, uint32_t msg_len,
                                        const uint64_t* d_msg_offsets, const uint64_t* d_rands, uint64_t n, uint8_t* d_partial, void* stream);
int mbls_verify_multiple_finish_device(mbls_ctx* ctx, const uint8_t* d_partials, uint64_t n_partials, uint8_t* d_result, uint32_t* d_status,
                                       void* stream);

/* MANY verify_multiple BATCHES IN ONE CALL. A consensus client calls verify_multiple_aggregate_signatures once per SMALL batch (one block's sets, one gossip
 * batch), and every entry above answers one bool per call -- a call is a latency chain of a few milliseconds whatever its size. These entries take B batches
 * over n_sets sets laid out back to back -- batch b owns the sets [batch_offsets[b], batch_offsets[b+1]) (n_batches + 1 offsets starting at 0) or
 * sets_per_batch each when the table is NULL (n_sets must then be n_batches x sets_per_batch) -- and answer per batch:
 *   results[b] = exactly what mbls_verify_multiple_aggregate_signatures returns for batch b's sets with batch b's scalars (an empty batch: 1);
 *   status[b] (optional) = the status word mbls_verify_multiple_aggregate_signatures_device writes for that batch (the OR of its sets' MBLS_ST_* bits; an empty
 *     batch: 0), PLUS MBLS_ST_PAIRING_FAILED exactly where the pairing check itself is what rejects the batch: results[b] = 0 and none of the rejecting bits
 *     (MBLS_ST_BAD_SIG_ENCODING, MBLS_ST_SIG_NOT_IN_G2, MBLS_ST_BAD_PK_ENCODING, MBLS_ST_BAD_MSG_RANGE, MBLS_ST_BAD_SCALAR) is set. (The one-batch entries
 *     report a failed pairing check through the bool only.)
 * No value crosses a batch boundary -- not a signature sum, not a product, not a status bit: a bad batch rejects itself and nothing else. The per-set work is
 * the one-batch entries' (one lane per set); the sum of a batch's blinded signatures and the product of its pairings are per-batch trees, the B (S_b, -G1)
 * pairs ride the sets' Miller launch, and every batch gets its own final exponentiation. n_batches = 0 (with n_sets = 0): MBLS_OK, nothing written.
 * d_rands / rands: one NONZERO scalar per set (see above); NULL is MBLS_ERR_ARGUMENT, a zero scalar rejects its batch (MBLS_ST_BAD_SCALAR).
 * The *_device forms ONLY ENQUEUE and order their use of the workspace against other calls like their neighbours. Keys per set: d_apks96 (one 96-byte aggregate key
 * per set) or, when that is NULL, wire-format keys d_pks / pk_format / d_pk_offsets / k as in mbls_verify_multiple_sets_device; the indexed form names them in a
 * resident key table as mbls_verify_multiple_sets_indexed_device does. Messages: msg_len bytes each or through d_msg_offsets (n_sets + 1 entries). A DEVICE-SIDE
 * batch table is not seen by the host: a range that runs backwards or ends beyond n_sets, and every range that shares a set with another, rejects the batches
 * involved (MBLS_ST_BAD_PK_ENCODING in their words) and never becomes a read outside the call's buffers; batches with sound ranges of their own are not touched.
 * Workspace: n_sets + 2 n_batches items (2 n_sets for calls of at most half a round, if that is more); mbls_ctx_reserve beforehand keeps allocation out of the call. */
int mbls_verify_multiple_batches_device(mbls_ctx* ctx, const uint8_t* d_sigs96, const uint8_t* d_apks96, const uint8_t* d_pks, int pk_format,
                                        const uint32_t* d_pk_offsets, uint32_t k, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_msg_offsets,
                                        const uint64_t* d_rands, uint64_t n_sets, const uint32_t* d_batch_offsets, uint32_t sets_per_batch, uint64_t n_batches,
                                        uint8_t* d_results, uint32_t* d_status, void* stream);
int mbls_verify_multiple_batches_indexed_device(mbls_ctx* ctx, const mbls_keytable* t, const uint8_t* d_sigs96, const uint32_t* d_key_idx, const uint32_t* d_offsets,
                                                uint32_t k, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_msg_offsets, const uint64_t* d_rands,
                                                uint64_t n_sets, const uint32_t* d_batch_offsets, uint32_t sets_per_batch, uint64_t n_batches, uint8_t* d_results,
                                                uint32_t* d_status, void* stream);
/* host buffers (aggregate keys, as mbls_verify_multiple_aggregate_signatures); the tables are validated on the host: batch_offsets must start at 0, be
 * non-decreasing and end at n_sets, msg_offsets as everywhere -- MBLS_ERR_ARGUMENT otherwise, nothing enqueued */
int mbls_verify_multiple_batches(mbls_ctx* ctx, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs, uint32_t msg_len, const uint64_t* msg_offsets,
                                 const uint64_t* rands, uint64_t n_sets, const uint32_t* batch_offsets, uint32_t sets_per_batch, uint64_t n_batches,
                                 uint8_t* results, uint32_t* status);
/* The reference's order (see mbls_verify_multiple_aggregate_signatures_rng), generalised: the signatures of ALL batches are decoded and tested first, the host reads
 * the verdicts, and `draw` is called AT MOST ONCE for, batch after batch in order, the scalars of the sets in front of that batch's first signature outside G2 (all
 * of the batch's sets when there is none) -- the sequence of draws n_batches consecutive reference calls sharing one generator would make, handed out in set
 * order. No second subgroup test afterwards. results[b] as above. */
int mbls_verify_multiple_batches_rng(mbls_ctx* ctx, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs, uint32_t msg_len, const uint64_t* msg_offsets,
                                     uint64_t n_sets, const uint32_t* batch_offsets, uint32_t sets_per_batch, uint64_t n_batches, uint8_t* results,
                                     mbls_scalar_source draw, void* user);

/* WHICH SETS OF A REJECTED BATCH. A client that gets results[b] = 0 must know which sets to drop; a second call over the rejected batches' sets would hash the
 * same messages, decode, subgroup-test and blind the same signatures and blind the same keys again, behind a second host round trip. The _locate entries answer
 * per set in the SAME call: arguments, table validation, MBLS_ERR_ARGUMENT cases, n_batches = 0 and empty batches are those of the corresponding
 * mbls_verify_multiple_batches* entry, plus d_set_results (n_sets bytes, REQUIRED: NULL is MBLS_ERR_ARGUMENT, nothing written) and d_set_status (n_sets words,
 * optional). The *_device forms ONLY ENQUEUE -- no host synchronisation anywhere; in particular the number of sets to examine is never read back.
 * CONTRACT.
 *  1. d_results[b] / d_status[b] are byte for byte what mbls_verify_multiple_batches_device writes for the same inputs.
 *  2. Every set of an ACCEPTED batch (d_results[b] = 1) gets d_set_results[i] = 1. A passing batch is NOT EXAMINED set by set: the batch check is the security
 *     statement verify_multiple makes (reference src/aggregates.rs:261-316), and sets whose errors cancel in it exist only with the blinding's probability 2^-63 --
 *     examining them would add cost to every call for no statement the function makes.
 *  3. Every set of a REJECTED batch gets exactly what mbls_verify_multiple_batches_device returns for the one-set batch {i} with the scalar rands[i]: the reject
 *     mask is verify_multiple's on the set's OWN word -- an undecodable signature, a signature outside G2, a bad key, a bad message range or a zero scalar give 0
 *     without a pairing --, otherwise the set passes exactly when FE(ML([r_i] apk_i, H(m_i)) . ML(-G1, [r_i] sig_i)) = 1 (an infinite key with an infinite
 *     signature: 1, as that entry gives).
 *  4. d_set_status[i] = the set's own MBLS_ST_* bits as phase one found them (the one-set batch's status word), with MBLS_ST_PAIRING_FAILED added exactly where the
 *     set was examined and its own pairing check is what rejects it.
 *  5. DEVICE-SIDE batch table: a set that no sound batch owns -- its range runs backwards or ends beyond n_sets, shares a set with another range, or no range
 *     covers the set -- gets 0 and MBLS_ST_BAD_PK_ENCODING (the bit the entries above use for table faults). Nothing is read outside the call's buffers, and the sets
 *     of sound batches are not touched by their neighbours' faults.
 *  6. The _rng form draws exactly as mbls_verify_multiple_batches_rng does. A set at or behind its batch's first signature outside G2 has no scalar (the reference
 *     never draws one): 0, and the status the signature phase found. Only sets with a scalar can be examined.
 * MECHANISM. Phase one is mbls_verify_multiple_batches_device's, with set i's blinded signature (as the pair ([r_i] sig_i, -G1)) and its Miller value f_i copied to
 * a shadow item before the per-batch trees overwrite them. Behind the per-batch tail one lane per set answers every set that needs no pairing and flags the rest;
 * the flagged sets walk one one-pair Miller loop, one product and one final exponentiation each, on the kernels' usual lane forms (lane pairs up to half a round,
 * rounds above one). Waves without a flagged set return at once.
 * WORKSPACE: 2 n_sets + 2 n_batches items (3 n_sets for calls of at most half a round whose message phase runs on lane pairs, if that is more): what
 * mbls_plan_locate_workspace_items returns -- a pure function; mbls_ctx_reserve(ctx, that) beforehand keeps allocation out of the call. The entries reserve once,
 * before the first kernel.
 * NOT PROVIDED: a wave-engine form of phase two for very small calls, locate forms of the mbls_multi handle and of the stream (the shared-message entries have
 * theirs: mbls_verify_multiple*_shared_msgs_locate* below). */
uint64_t mbls_plan_locate_workspace_items(const mbls_limits* limits, uint64_t n_sets, uint64_t n_batches);
int mbls_verify_multiple_batches_locate_device(mbls_ctx* ctx, const uint8_t* d_sigs96, const uint8_t* d_apks96, const uint8_t* d_pks, int pk_format,
                                               const uint32_t* d_pk_offsets, uint32_t k, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_msg_offsets,
                                               const uint64_t* d_rands, uint64_t n_sets, const uint32_t* d_batch_offsets, uint32_t sets_per_batch, uint64_t n_batches,
                                               uint8_t* d_results, uint32_t* d_status, uint8_t* d_set_results, uint32_t* d_set_status, void* stream);
int mbls_verify_multiple_batches_locate_indexed_device(mbls_ctx* ctx, const mbls_keytable* t, const uint8_t* d_sigs96, const uint32_t* d_key_idx,
                                                       const uint32_t* d_offsets, uint32_t k, const uint8_t* d_msgs, uint32_t msg_len, const uint64_t* d_msg_offsets,
                                                       const uint64_t* d_rands, uint64_t n_sets, const uint32_t* d_batch_offsets, uint32_t sets_per_batch,
                                                       uint64_t n_batches, uint8_t* d_results, uint32_t* d_status, uint8_t* d_set_results, uint32_t* d_set_status,
                                                       void* stream);
/* host buffers, aggregate keys; validation as mbls_verify_multiple_batches */
int mbls_verify_multiple_batches_locate(mbls_ctx* ctx, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs, uint32_t msg_len,
                                        const uint64_t* msg_offsets, const uint64_t* rands, uint64_t n_sets, const uint32_t* batch_offsets, uint32_t sets_per_batch,
                                        uint64_t n_batches, uint8_t* results, uint32_t* status, uint8_t* set_results, uint32_t* set_status);
/* the reference's draw order (contract item 6) */
int mbls_verify_multiple_batches_locate_rng(mbls_ctx* ctx, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs, uint32_t msg_len,
                                            const uint64_t* msg_offsets, uint64_t n_sets, const uint32_t* batch_offsets, uint32_t sets_per_batch, uint64_t n_batches,
                                            uint8_t* results, uint8_t* set_results, uint32_t* set_status, mbls_scalar_source draw, void* user);

/* verify_multiple OVER A SHARED MESSAGE LIST: ONE MILLER LOOP PER MESSAGE. The sets come in the caller's order, each with one uint32 naming its message in a
 * list of the shape of the `_shared_msgs` entries above (msgs, msg_len or msg_offsets[n_msgs + 1], n_msgs, msg_idx[n]). Pairings are bilinear in the key argument
 * over all of E(Fp), so  prod_i e([r_i] apk_i, H(m_i)) = prod_j e(sum_{i: msg(i) = j} [r_i] apk_i, H(m_j)):  n sets over M distinct messages need M hashes and M
 * Miller loops instead of n of each. The list is hashed once (the path of the entries above); the blinded keys are grouped by message ON THE DEVICE (count, scan,
 * scatter; mbls_vms.h), summed per message (k_g1_seg_tree_d) and each sum walks one Miller loop with its message's point. [r] apk, [r] sig, the signatures' sum
 * and the single final exponentiation are mbls_verify_multiple_aggregate_signatures_device's.
 * CONTRACT. *d_result is byte for byte what mbls_verify_multiple_aggregate_signatures_device writes for the same signatures, keys and scalars with each set's
 * message spelled out. *d_status (optional) equals that entry's word in the bits that reject a batch -- MBLS_ST_BAD_SIG_ENCODING, MBLS_ST_SIG_NOT_IN_G2,
 * MBLS_ST_BAD_PK_ENCODING, MBLS_ST_BAD_MSG_RANGE, MBLS_ST_BAD_SCALAR --; the other bits (MBLS_ST_APK_INFINITY, MBLS_ST_PK_INFINITY, MBLS_ST_NO_KEYS) are the OR
 * over the sets as the key phase reports them and equal it too; MBLS_ST_PAIRING_FAILED is never set (a failed pairing check shows in the bool only, as there).
 * n = 0: result 1, status 0. rands == NULL: MBLS_ERR_ARGUMENT. A zero scalar rejects (MBLS_ST_BAD_SCALAR). Listed messages no set names are harmless (hashed,
 * and their Miller item has an infinite key and contributes 1). Two list entries with equal bytes are two groups.
 * DEVICE ENTRIES (enqueue only): msg_idx[i] >= n_msgs (n_msgs = 0 included) rejects the check with MBLS_ST_BAD_MSG_RANGE -- such a set joins no group --; a listed
 * message whose range runs backwards or is 2^32 bytes or more rejects the check exactly when a set names it. Neither becomes a read outside the call's buffers,
 * and every slot a Miller loop reads has been written by this call. HOST ENTRIES refuse both with MBLS_ERR_ARGUMENT before anything is queued (outputs untouched).
 * ROUTING (mbls_ctx_set_vm_grouping; mbls_ctx_reset_tuning restores 0): 0 auto -- grouped when 2 n_msgs <= n --, 1 always grouped, 2 never: the list is still
 * hashed once and every set copies its message's point (k_h_gather) and walks its own Miller loop -- the route for lists with almost as many messages as sets.
 * ALLOCATION: workspace (mbls_plan_verify_multiple_shared_msgs_workspace_items) and message table are reserved once, before the first kernel;
 * mbls_ctx_reserve and mbls_ctx_reserve_msgs beforehand keep allocation out of the call.
 * OUT OF SCOPE: the mbls_multi handle, the verification stream, the shard form (d_partial) and sets given by wire-format keys (d_pks) take per-set messages only. */
int mbls_ctx_set_vm_grouping(mbls_ctx* ctx, int mode);
/* Routing as data (pure: no GPU, no context; the SAME function the entries act on). route; the list hash as mbls_plan_batch_shared_msgs states it (list_*,
 * table_entries); miller_items = the one-pair Miller loops (grouped: max(n_msgs, 1); per set: n), walked one WAVE each (miller = MBLS_PAIRING_WAVE) up to
 * coop_max_items / 2, else as miller_rounds whole rounds of one lane each followed by miller_rest_items in the form `miller` (MBLS_PAIRING_LANES2 up to half a
 * round, MBLS_PAIRING_LANE); tree_levels = the levels of the per-message key sums a DEVICE entry enqueues (all n sets may share a message: vmb_levels(n); the
 * host entries count the longest group and enqueue fewer); chains_beside / sig_lane_pairs: the per-set chains as mbls_verify_multiple_aggregate_signatures_device
 * shapes them (side by side up to half a round; two lanes per signature up to coop_max_items / 2); workspace_items = what the call reserves.
 * MBLS_ERR_ARGUMENT for n = 0, a mode outside 0..2 or null pointers (the workspace function then returns 0). */
enum { MBLS_VM_ROUTE_PER_SET = 0, MBLS_VM_ROUTE_GROUPED = 1 };
typedef struct mbls_vm_shared_msgs_plan {
    uint32_t route, list_message, list_pieces, miller, tree_levels, chains_beside, sig_lane_pairs, reserved;
    uint64_t list_piece_items, list_workspace_items, table_entries, miller_items, miller_rounds, miller_rest_items, workspace_items;
} mbls_vm_shared_msgs_plan;
int mbls_plan_verify_multiple_shared_msgs(const mbls_limits* limits, uint64_t n, uint64_t n_msgs, int mode, mbls_vm_shared_msgs_plan* out);
uint64_t mbls_plan_verify_multiple_shared_msgs_workspace_items(const mbls_limits* limits, uint64_t n, uint64_t n_msgs, int mode);
int mbls_verify_multiple_shared_msgs_device(mbls_ctx* ctx, const uint8_t* d_sigs96, const uint8_t* d_apks96, const uint8_t* d_msgs, uint32_t msg_len,
                                            const uint64_t* d_msg_offsets, uint64_t n_msgs, const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n,
                                            uint8_t* d_result, uint32_t* d_status, void* stream);
/* keys by index into a resident key table, as mbls_verify_multiple_sets_indexed_device names them (the deployment's form) */
int mbls_verify_multiple_sets_indexed_shared_msgs_device(mbls_ctx* ctx, const mbls_keytable* t, const uint8_t* d_sigs96, const uint32_t* d_key_idx,
                                                         const uint32_t* d_offsets, uint32_t k, const uint8_t* d_msgs, uint32_t msg_len,
                                                         const uint64_t* d_msg_offsets, uint64_t n_msgs, const uint32_t* d_msg_idx, const uint64_t* d_rands,
                                                         uint64_t n, uint8_t* d_result, uint32_t* d_status, void* stream);
/* host buffers; returns a status code, the bool through *result (and the status word through *status, optional), like mbls_verify_multiple_batches */
int mbls_verify_multiple_shared_msgs(mbls_ctx* ctx, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs, uint32_t msg_len,
                                     const uint64_t* msg_offsets, uint64_t n_msgs, const uint32_t* msg_idx, const uint64_t* rands, uint64_t n,
                                     uint8_t* result, uint32_t* status);
/* the reference's order exactly as mbls_verify_multiple_aggregate_signatures_rng keeps it: signatures decoded and tested first, `draw` called at most once for
 * the sets in front of the first bad signature (*result = 0 then), no second subgroup test */
int mbls_verify_multiple_shared_msgs_rng(mbls_ctx* ctx, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs, uint32_t msg_len,
                                         const uint64_t* msg_offsets, uint64_t n_msgs, const uint32_t* msg_idx, uint64_t n, uint8_t* result,
                                         mbls_scalar_source draw, void* user);

/* WHICH SETS OF A REJECTED SHARED-MESSAGE CALL. The two features above composed: a caller of mbls_verify_multiple*_shared_msgs who gets 0 would otherwise spell
 * every set's message out again and run mbls_verify_multiple_batches_locate* over all n sets -- n hashes and n Miller loops, behind a second host round trip, on
 * the path an attacker triggers with one bad signature. The _locate entries answer per set in the SAME call: arguments, validation, n = 0, rands == NULL, what the
 * host entries refuse and the routing (mbls_ctx_set_vm_grouping) are those of the corresponding entry above, plus d_set_results (n bytes, REQUIRED: NULL is
 * MBLS_ERR_ARGUMENT, nothing written) and d_set_status (n words, optional). The *_device forms ONLY ENQUEUE -- no host synchronisation anywhere; in particular the
 * number of sets to examine is never read back.
 * CONTRACT.
 *  1. *d_result / *d_status are byte for byte what mbls_verify_multiple_shared_msgs_device writes for the same inputs and the same grouping mode. Calls without
 *     _locate do not change in any launch or byte.
 *  2. An ACCEPTED call gives every set 1. A passing batch is NOT EXAMINED set by set (item 2 of the contract above: the batch check is the security statement).
 *  3. A REJECTED call gives set i what the one-set call {i} with the scalar rands[i] and its message spelled out returns: a rejecting bit of verify_multiple's
 *     mask in the set's OWN word gives 0 without a pairing; otherwise the set passes exactly when FE(ML([r_i] apk_i, H(m_{idx(i)})) . ML(-G1, [r_i] sig_i)) = 1
 *     (an infinite key with an infinite signature: 1, as there).
 *  4. d_set_status[i] = the set's own MBLS_ST_* bits as phase one found them, with MBLS_ST_PAIRING_FAILED added exactly where the set's own check rejects it.
 *  5. MESSAGE FAULTS on device-side lists give the set 0 with MBLS_ST_BAD_MSG_RANGE in its own word and no pairing: msg_idx[i] >= n_msgs (n_msgs = 0 included),
 *     and a set that names a listed message whose range runs backwards or is 2^32 bytes or more (the grouped route reports such a message in the call's word
 *     only; the mark step looks the message's flag up through msg_idx[i]). Nothing is read outside the call's buffers; a set naming a sound message is untouched
 *     by its neighbours' faults.
 *  6. The _rng form draws exactly as mbls_verify_multiple_shared_msgs_rng does. A set at or behind the first signature outside G2 has no scalar (the reference
 *     never draws one): 0, and the status the signature phase found. Only sets with a scalar -- those in front of it -- can be examined.
 *  7. Per-set answers are deterministic: positions inside a group vary from run to run with the atomics, and nothing per set depends on them.
 * MECHANISM. Per-set route (mode 2; auto when 2 n_msgs > n): a Miller value per set exists, and the scheme is the one above with the call as the one batch --
 * ([r_i] sig_i, -G1) and f_i kept in ONE shadow item per set, mark, one-pair loop, product, final exponentiation. Grouped route: f_i is never computed, the heads
 * and per-message trees overwrite the sets' blinded keys and the signatures' tree their slot S, so each set gets TWO shadow items: A(i) keeps [r_i] apk_i (copied
 * behind the blinding, before the grouping), B(i) the pair ([r_i] sig_i, -G1). Behind the tail one lane per set applies the rule (mbls_vsl.h: call verdict, own
 * word, message flag through msg_idx) and copies a candidate's H(m) from the message table into A(i); one Miller launch walks the 2 n shadow items (cut at rounds,
 * lane pairs up to half a round; waves without a candidate return after one ballot), a tree level with half = n forms A(i) . B(i), and a final exponentiation
 * per candidate decides on the set's own word.
 * WORKSPACE: what the entry above reserves (mbls_plan_verify_multiple_shared_msgs_workspace_items) plus n items on the per-set route, 2 n on the grouped one,
 * behind everything phase one uses: mbls_plan_verify_multiple_shared_msgs_locate_workspace_items -- a pure function (0 for n = 0, a mode outside 0..2 or null
 * limits). Reserved once, before the first kernel; the _rng form reserves before its first half.
 * NOT PROVIDED: a wave-engine form of phase two, compaction of the candidates, a per-message first level that narrows the candidates to the bad groups; the
 * mbls_multi handle, the stream, the shard form and wire-key sets (as for the entries above). */
uint64_t mbls_plan_verify_multiple_shared_msgs_locate_workspace_items(const mbls_limits* limits, uint64_t n, uint64_t n_msgs, int mode);
int mbls_verify_multiple_shared_msgs_locate_device(mbls_ctx* ctx, const uint8_t* d_sigs96, const uint8_t* d_apks96, const uint8_t* d_msgs, uint32_t msg_len,
                                                   const uint64_t* d_msg_offsets, uint64_t n_msgs, const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n,
                                                   uint8_t* d_result, uint32_t* d_status, uint8_t* d_set_results, uint32_t* d_set_status, void* stream);
int mbls_verify_multiple_sets_indexed_shared_msgs_locate_device(mbls_ctx* ctx, const mbls_keytable* t, const uint8_t* d_sigs96, const uint32_t* d_key_idx,
                                                                const uint32_t* d_offsets, uint32_t k, const uint8_t* d_msgs, uint32_t msg_len,
                                                                const uint64_t* d_msg_offsets, uint64_t n_msgs, const uint32_t* d_msg_idx, const uint64_t* d_rands,
                                                                uint64_t n, uint8_t* d_result, uint32_t* d_status, uint8_t* d_set_results, uint32_t* d_set_status,
                                                                void* stream);
/* host buffers; validation as mbls_verify_multiple_shared_msgs */
int mbls_verify_multiple_shared_msgs_locate(mbls_ctx* ctx, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs, uint32_t msg_len,
                                            const uint64_t* msg_offsets, uint64_t n_msgs, const uint32_t* msg_idx, const uint64_t* rands, uint64_t n,
                                            uint8_t* result, uint32_t* status, uint8_t* set_results, uint32_t* set_status);
/* the reference's draw order (contract item 6) */
int mbls_verify_multiple_shared_msgs_locate_rng(mbls_ctx* ctx, const uint8_t* sigs96, const uint8_t* apks96, const uint8_t* msgs, uint32_t msg_len,
                                                const uint64_t* msg_offsets, uint64_t n_msgs, const uint32_t* msg_idx, uint64_t n, uint8_t* result,
                                                uint8_t* set_results, uint32_t* set_status, mbls_scalar_source draw, void* user);

/* verify_multiple OVER THE RESIDENT MESSAGE TABLE, LOCATED PER SET. The shared-message entries above with the messages named by index into a resident message
 * table (mbls_msgtable_*) in place of a list the call carries: NOTHING IS HASHED, no call table is written. d_msg_idx[n] / msg_idx[n] are TABLE indices. The table
 * is read at the size T it has when the call is enqueued (under the context's lock, as the per-item `_msgtable` entries read it), and its last append on another
 * stream is awaited on the caller's stream before the call's streams fork.
 * A resident table outlives calls and may hold far more entries than one call names, so the table is not treated as the list: the grouping runs over the T
 * entries (count, scan, scatter and per-entry key sums as above), then the entries that are NAMED are compacted on the device in increasing table index
 * (mbls_vmt.h: flag, scan, named), and the Miller items are built from those -- one per named entry, D of them. D stays on the device and is never read back.
 * ROUTING AND SIZING (mbls_ctx_set_vm_grouping as above). The Miller phase is sized by `bound`, what the host knows about D: the DEVICE entries never see the
 * indices and use bound = min(n, T); the HOST entries (_rng) count D and the longest group exactly. Everything else is the rule above with bound in place of
 * n_msgs: auto groups when 2 bound <= n, miller_items = max(bound, 1), the Miller form follows miller_items, tree levels follow the longest group (host) or n
 * (device). Miller items at or above D hold the private entry and the point at infinity and contribute 1; waves that hold no item below D return before any
 * arithmetic, on the wave form and on the lane forms. Per-set route: one gather straight from the resident table.
 * mbls_plan_verify_multiple_msgtable is the pure function the entries act on (named = 0: "not known", the device entries' case; otherwise D as a host entry
 * counts it). It fills mbls_vm_shared_msgs_plan with the list fields (list_*, table_entries) zero. MBLS_ERR_ARGUMENT for n = 0, a mode outside 0..2 or null
 * pointers; the workspace functions then return 0.
 * CONTRACT: that of the shared-message entries and their _locate forms with "list" read as "table": result and rejecting status bits of
 * mbls_verify_multiple_aggregate_signatures_device on the spelled-out messages; per set, what the one-set call returns. An index at or above T (an empty table:
 * every index) rejects its set with MBLS_ST_BAD_MSG_RANGE on the device entries and is refused (MBLS_ERR_ARGUMENT, nothing queued, outputs untouched) by the
 * host entries; an entry flagged at its append (a bad range) rejects the call exactly when a set names it, and the _locate forms put the bit into the word of
 * exactly the sets that name it. n = 0: result 1. A table of another context: MBLS_ERR_ARGUMENT.
 * ALLOCATION: workspace (mbls_plan_verify_multiple_msgtable_workspace_items, _locate_workspace_items) and six words per table entry for the grouping, reserved
 * once before the first kernel; mbls_ctx_reserve beforehand keeps the workspace allocation out of the call.
 * OUT OF SCOPE: the verification stream (mbls_stream_*), the mbls_multi handle, the shard form (d_partial) and sets given by 48-byte wire-format keys. */
int mbls_plan_verify_multiple_msgtable(const mbls_limits* limits, uint64_t n, uint64_t table_size, uint64_t named, int mode, mbls_vm_shared_msgs_plan* out);
uint64_t mbls_plan_verify_multiple_msgtable_workspace_items(const mbls_limits* limits, uint64_t n, uint64_t table_size, uint64_t named, int mode);
uint64_t mbls_plan_verify_multiple_msgtable_locate_workspace_items(const mbls_limits* limits, uint64_t n, uint64_t table_size, uint64_t named, int mode);
int mbls_verify_multiple_msgtable_device(mbls_ctx* ctx, const uint8_t* d_sigs96, const uint8_t* d_apks96, const mbls_msgtable* mt, const uint32_t* d_msg_idx,
                                         const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status, void* stream);
/* keys by index into a resident key table, as mbls_verify_multiple_sets_indexed_device names them */
int mbls_verify_multiple_sets_indexed_msgtable_device(mbls_ctx* ctx, const mbls_keytable* t, const uint8_t* d_sigs96, const uint32_t* d_key_idx,
                                                      const uint32_t* d_offsets, uint32_t k, const mbls_msgtable* mt, const uint32_t* d_msg_idx,
                                                      const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status, void* stream);
/* host buffers, the reference's draw order as mbls_verify_multiple_shared_msgs_rng keeps it */
int mbls_verify_multiple_msgtable_rng(mbls_ctx* ctx, const uint8_t* sigs96, const uint8_t* apks96, const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n,
                                      uint8_t* result, mbls_scalar_source draw, void* user);
/* the _locate forms: d_set_results (n bytes) REQUIRED, d_set_status (n words) optional; *d_result / *d_status byte for byte the entry above's under the same mode */
int mbls_verify_multiple_msgtable_locate_device(mbls_ctx* ctx, const uint8_t* d_sigs96, const uint8_t* d_apks96, const mbls_msgtable* mt, const uint32_t* d_msg_idx,
                                                const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status, uint8_t* d_set_results,
                                                uint32_t* d_set_status, void* stream);
int mbls_verify_multiple_sets_indexed_msgtable_locate_device(mbls_ctx* ctx, const mbls_keytable* t, const uint8_t* d_sigs96, const uint32_t* d_key_idx,
                                                             const uint32_t* d_offsets, uint32_t k, const mbls_msgtable* mt, const uint32_t* d_msg_idx,
                                                             const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status, uint8_t* d_set_results,
                                                             uint32_t* d_set_status, void* stream);
int mbls_verify_multiple_msgtable_locate_rng(mbls_ctx* ctx, const uint8_t* sigs96, const uint8_t* apks96, const mbls_msgtable* mt, const uint32_t* msg_idx,
                                             uint64_t n, uint8_t* result, uint8_t* set_results, uint32_t* set_status, mbls_scalar_source draw, void* user);

/* verify_multiple OVER COMMITTEE BITFIELDS AND THE RESIDENT MESSAGE TABLE. A consensus client verifies gossip with verify_multiple_aggregate_signatures, and a
 * gossip batch mixes two kinds of set: an aggregate over a committee's bitfield, and sets under ONE validator key (a SignedAggregateAndProof's selection proof and
 * its aggregator's signature, an unaggregated attestation). These entries are mbls_verify_multiple_sets_indexed_msgtable[_locate]_device with `d_key_idx,
 * d_offsets, k` replaced by `committees, d_cmt_idx, d_bits, bits_stride` -- the key table is the one the committee table is bound to --, and take both kinds in
 * one call. Set i is described by the word cmt_idx[i] and the bits_stride bytes at bits + bits_stride * i (csrc/mbls_vmc.h):
 *   bit 31 clear: a COMMITTEE set. The word is a committee id, the bytes its SSZ bitfield, every rule the committee section's above: bits at or above the
 *     committee's size are ignored, the route is cmt_route's under mbls_ctx_set_committee_route, an id at or above the count lists the one index 0xFFFFFFFF.
 *   bit 31 set (MBLS_VM_SET_SINGLE_KEY | index): a SINGLE-KEY set. The low 31 bits are an index into the key table; the set's key list is that one index on the
 *     direct route and its bitfield bytes are NOT READ (they are still bits_stride bytes of the buffer). An index at or above the key table's size rejects the
 *     set through the key sum (MBLS_ST_BAD_PK_ENCODING) like any index outside the table; 0xFFFFFFFF therefore still rejects.
 * The committee entries of the section above do not change: they keep treating a bit-31 id as one that names no committee.
 * KEY PHASE. k_vmc_expand (one wave per set) writes every set's index list -- the selected members, the missing ones on the complement route, or the one key --,
 * count and route word; the committee entries' key sum over those lists leaves each set's sum where the indexed key sum leaves it. Everything behind it --
 * blinding, grouping by table entry, heads, Miller loops, tail, both phase-two routes of the _locate forms -- is the _msgtable entries' above, unchanged.
 * CONTRACT. *d_result, *d_status, and for the _locate forms every byte of d_set_results and every word of d_set_status, are those of
 * mbls_verify_multiple_sets_indexed_msgtable[_locate]_device on the same signatures, scalars and message indices with every set's signers spelled out in member
 * order through a ragged offset table (a single-key set spells out as its one index), under every mode of mbls_ctx_set_vm_grouping and of
 * mbls_ctx_set_committee_route. The status bits of the key phase are therefore verify_multiple's: MBLS_ST_BAD_PK_ENCODING and MBLS_ST_PK_INFINITY of the LISTED
 * members of an ineligible committee (which always goes direct), as the indexed key sum reports them. Like those entries -- and unlike fast_aggregate_verify --
 * the key phase does not flag an empty bitfield or a sum at infinity (no MBLS_ST_NO_KEYS, no MBLS_ST_APK_INFINITY): such a set's key is the point at infinity,
 * its pairing contributes 1, and the call is rejected through the product unless its signature is the point at infinity too.
 * ARGUMENTS: the committee entries' checks (one context for all three tables, the key table alive, bits_stride a multiple of 4 that covers
 * mbls_committees_max_members, d_bits 4-byte aligned) and the _msgtable entries' (d_rands and, for _locate, d_set_results not NULL); otherwise MBLS_ERR_ARGUMENT.
 * n = 0 answers as mbls_verify_multiple_msgtable_device does (result 1, status 0). The tables are read at the sizes they have when the call is enqueued.
 * HOST ENTRIES (_rng) keep the reference's order exactly as mbls_verify_multiple_msgtable_rng does: signatures decoded and tested first, `draw` called at most
 * once, for the sets in front of the first bad signature. They refuse with MBLS_ERR_ARGUMENT, nothing queued and the outputs untouched: a committee id at or
 * above the count, a single-key index at or above the key table's size, a message index at or above the message table's size.
 * ORDERING AND ALLOCATION are the committee section's: the list scratch -- n x (largest committee) words plus two words per set -- is reserved for the n sets
 * before the first kernel of the call (mbls_ctx_reserve_committee_items beforehand keeps that out of the call); the last appends to the committee table, its key
 * table and the message table are awaited on the caller's stream before any side stream has work, and no fallible step is left once one has.
 * PLANNING. Routing and workspace are mbls_plan_verify_multiple_msgtable, _workspace_items and _locate_workspace_items, UNCHANGED: the committee source adds
 * no workspace item (its scratch is the committee entries').
 * OUT OF SCOPE: the verification stream, the shared-list and per-set message forms over committees, the mbls_multi
 * handle and the shard form, a device-pointer append. (fast_aggregate_verify over sets that span several committees: "committee spans" above; verify_multiple
 * over such sets: the section below; many batches per call over committees: mbls_verify_multiple_batches_committee_msgtable*, below.) */
#define MBLS_VM_SET_SINGLE_KEY 0x80000000u
int mbls_verify_multiple_committee_msgtable_device(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* d_sigs96, const uint32_t* d_cmt_idx,
                                                   const uint8_t* d_bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* d_msg_idx,
                                                   const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status, void* stream);
int mbls_verify_multiple_committee_msgtable_locate_device(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* d_sigs96, const uint32_t* d_cmt_idx,
                                                          const uint8_t* d_bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* d_msg_idx,
                                                          const uint64_t* d_rands, uint64_t n, uint8_t* d_result, uint32_t* d_status, uint8_t* d_set_results,
                                                          uint32_t* d_set_status, void* stream);
int mbls_verify_multiple_committee_msgtable_rng(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* sigs96, const uint32_t* cmt_idx,
                                                const uint8_t* bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n,
                                                uint8_t* result, mbls_scalar_source draw, void* user);
int mbls_verify_multiple_committee_msgtable_locate_rng(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* sigs96, const uint32_t* cmt_idx,
                                                       const uint8_t* bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n,
                                                       uint8_t* result, uint8_t* set_results, uint32_t* set_status, mbls_scalar_source draw, void* user);

/* verify_multiple OVER COMMITTEE SPANS AND THE RESIDENT MESSAGE TABLE. A block is imported through verify_multiple_aggregate_signatures: up to 8 attestations that
 * each name up to 64 committees and carry one field over all of them (EIP-7549), the sync aggregate (one 512-member committee) and a few sets under one validator
 * key (proposer signature, randao reveal, exits). These entries are the _committee_msgtable entries above with `d_cmt_idx` replaced by the span entries'
 * `d_cmt_ids, n_cmt_ids, d_cmt_off` (csrc/mbls_vcs.h). Set i names cmt_ids[cmt_off[i] .. cmt_off[i + 1]) and the bits_stride bytes at bits + bits_stride * i; every
 * rule of "committee spans" applies unchanged: absolute offsets, q <= MBLS_SPAN_MAX_COMMITTEES, SSZ bit order, bits at or above M ignored, bits_stride a multiple
 * of 4, d_bits 4-byte aligned, the same id twice allowed, every segment on its own route from cmt_route under mbls_ctx_set_committee_route.
 * A SINGLE-KEY set is a set of EXACTLY ONE id with bit 31 set (MBLS_VM_SET_SINGLE_KEY | key index): its list is that one index on the direct route, its field bytes
 *   are NOT READ, an index outside the key table rejects the set through the key sum. A bit-31 id inside a set of two or more ids names no committee: malformed.
 * MALFORMED SETS: an id at or above the committee count, q > 64, offsets that run backwards or past n_cmt_ids, M > 8 * bits_stride. DEVICE entries reject such a
 *   set like a set that lists the key index 0xFFFFFFFF, reading in the span section's order (offsets before ids, ids before records, M before the field). HOST
 *   entries (_rng) refuse the call with MBLS_ERR_ARGUMENT, nothing queued, the outputs untouched; so they do for a single-key index or a message index that names
 *   nothing. n = 0 answers as mbls_verify_multiple_msgtable_device does. The _rng entries keep the reference's draw order exactly as
 *   mbls_verify_multiple_committee_msgtable_rng does.
 * CONTRACT. *d_result, *d_status, and for _locate every set byte and every set word, equal mbls_verify_multiple_sets_indexed_msgtable[_locate]_device on the same
 *   signatures, scalars and message indices with every set's selected members spelled out in (segment, member) order -- under every mode of
 *   mbls_ctx_set_vm_grouping and mbls_ctx_set_committee_route and every split factor below. As above the key phase flags neither an empty selection nor a sum at
 *   infinity. A set of one plain committee returns what the _committee_msgtable entry returns. Everything behind the key sum is verify_multiple over the message
 *   table, unchanged.
 * KEY PHASE AND SPLIT. k_vcs_expand (one wave per set) leaves the span entries' direct list, missing list and record in the span scratch
 *   (mbls_ctx_reserve_committee_span_items, reserved for all n sets before the first kernel). With split factor P = 1 one lane per set sums both lists, as the
 *   span entries do: the throughput form. A block is a dozen sets, and one lane would walk a chain of up to 8 192 additions while the chip idles: with
 *   P in {2, 4, 8, 16} each list is cut into P chunks -- chunk p of L entries is [floor(p L / P), floor((p + 1) L / P)) --, 2 P n lanes sum one chunk each into
 *   workspace items BEHIND what the call reserves otherwise, and one lane per set adds the partial sums and the cached sums of the complement segments.
 *   mbls_ctx_set_vm_span_split(ctx, 0 | 1 | 2 | 4 | 8 | 16): 0 (default; mbls_ctx_reset_tuning) chooses by rule -- P = 1 above 4 096 sets or once 2 n reaches a
 *   round, else the largest P whose lanes fill at most half a round (4 P n <= round_items) and whose chunks of a full region (stride words =
 *   min(8 * bits_stride, 64 * mbls_committees_max_members)) hold at least 8 entries --; another value is the factor asked for, halved until 2 P n fits a round;
 *   anything else is MBLS_ERR_ARGUMENT. Measured (profiles/vm_committee_span_throughput.json): a block of 12 sets at 45 % participation 47.7 -> 6.5 ms.
 * PLANNING. mbls_plan_verify_multiple_span(limits, n, table_size, stride_words, locate, split_mode, &split, &workspace_items), without a GPU (the name leaves the
 *   "committee" out: the committee entries above have, and keep, no planning symbol of their own): the factor
 *   P a call takes, and the workspace items it reserves -- mbls_plan_verify_multiple_msgtable[_locate]_workspace_items(limits, n, table_size, 0, 0) plus 2 P n for
 *   P > 1 (nothing for P = 1: the one-lane form parks its intermediate point in the span scratch). Under mbls_ctx_set_vm_grouping other than 0 the first term is
 *   that function's under the mode.
 * OUT OF SCOPE: the verification stream, the shared-list and per-set message forms, the mbls_multi handle and the shard form, a device-pointer append,
 * splitting the chain of up to 64 cached sums. (Many such batches per call, one verdict per batch: mbls_verify_multiple_batches_committee_span_msgtable*, below.) */
int mbls_verify_multiple_committee_span_msgtable_device(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* d_sigs96, const uint32_t* d_cmt_ids,
                                                        uint64_t n_cmt_ids, const uint32_t* d_cmt_off, const uint8_t* d_bits, uint32_t bits_stride,
                                                        const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n, uint8_t* d_result,
                                                        uint32_t* d_status, void* stream);
int mbls_verify_multiple_committee_span_msgtable_locate_device(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* d_sigs96, const uint32_t* d_cmt_ids,
                                                               uint64_t n_cmt_ids, const uint32_t* d_cmt_off, const uint8_t* d_bits, uint32_t bits_stride,
                                                               const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n,
                                                               uint8_t* d_result, uint32_t* d_status, uint8_t* d_set_results, uint32_t* d_set_status, void* stream);
int mbls_verify_multiple_committee_span_msgtable_rng(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* sigs96, const uint32_t* cmt_ids,
                                                     uint64_t n_cmt_ids, const uint32_t* cmt_off, const uint8_t* bits, uint32_t bits_stride, const mbls_msgtable* mt,
                                                     const uint32_t* msg_idx, uint64_t n, uint8_t* result, mbls_scalar_source draw, void* user);
int mbls_verify_multiple_committee_span_msgtable_locate_rng(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* sigs96, const uint32_t* cmt_ids,
                                                            uint64_t n_cmt_ids, const uint32_t* cmt_off, const uint8_t* bits, uint32_t bits_stride,
                                                            const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n, uint8_t* result, uint8_t* set_results,
                                                            uint32_t* set_status, mbls_scalar_source draw, void* user);
int mbls_ctx_set_vm_span_split(mbls_ctx* ctx, int mode);
int mbls_plan_verify_multiple_span(const mbls_limits* limits, uint64_t n, uint64_t table_size, uint64_t stride_words, int locate, int split_mode,
                                             uint32_t* split, uint64_t* workspace_items);

/* MANY verify_multiple BATCHES PER CALL OVER COMMITTEE BITFIELDS AND THE RESIDENT MESSAGE TABLE. A consensus client verifies gossip in many small
 * verify_multiple_aggregate_signatures batches and retries a rejected batch set by set. These entries answer PER BATCH, with per-set location, on the cheapest
 * inputs the library has: the sets are those of mbls_verify_multiple_committee_msgtable[_locate]_device (`committees, d_sigs96, d_cmt_idx, d_bits, bits_stride, mt,
 * d_msg_idx, d_rands, n_sets`: committee set or single-key set, the route under mbls_ctx_set_committee_route, an id that names nothing lists 0xFFFFFFFF), the
 * batches those of mbls_verify_multiple_batches[_locate]_device (`d_batch_offsets` / `sets_per_batch`, `n_batches`, `d_results`, `d_status`, for _locate
 * `d_set_results` (required) and `d_set_status`); every rule of both sections holds unchanged, those about a faulty device-side batch table included.
 * max_groups (device entries): the caller's bound on the number of distinct (batch, table entry) pairs of the call; 0 makes no promise.
 * CONTRACT. d_results[b], d_status[b], and for _locate every byte of d_set_results and every word of d_set_status, equal
 *   mbls_verify_multiple_batches[_locate]_indexed_device on the same signatures, scalars and batch table with every set's signers spelled out in member order (a
 *   single-key set as its one index) and every set's message spelled out as the bytes of its table entry -- under every mode of mbls_ctx_set_vm_grouping, every mode
 *   of mbls_ctx_set_committee_route and every max_groups the call does not exceed. Items 1-6 of "WHICH SETS OF A REJECTED BATCH" therefore carry over. No value
 *   crosses a batch boundary. A message index at or above the table's size rejects its set, and with it its batch, with MBLS_ST_BAD_MSG_RANGE (device entries).
 *   The device entries only enqueue, nothing is read back, and every fallible step (reserves, table acquires) comes before the first kernel on a side stream.
 * ROUTING (mbls_ctx_set_vm_grouping: 0 auto, 1 grouped, 2 per set). bound = the smallest of n_sets, n_batches x table size, n_batches x sets_per_batch where that
 *   is given, and max_groups where that is nonzero (host entries: their exact count). The table-size term holds only where no batch can be larger than
 *   MBLS_VBG_MAX_SETS -- sets_per_batch, or n_sets under a ragged device-side table, is at most that --: a larger batch has one group per set. Auto groups when 2 x bound <= n_sets -- the rule of the shared-message
 *   entries, a count and not a measurement.
 *   PER SET: mbls_verify_multiple_batches' path with the key phase the committee entries' (k_vmc_expand, the committee key sum) and the message phase the gather
 *   from the table; n_sets + n_batches Miller items.
 *   GROUPED (csrc/mbls_vbg.h, csrc/mbls_vbg.hip): inside a batch prod_i e([r_i] apk_i, H(m_i)) = prod_j e(sum_{i: m_i = j} [r_i] apk_i, H(m_j)), so a batch walks
 *   one Miller loop per DISTINCT entry it names plus its signature pair: n_batches + bound Miller items, of which n_batches + (the groups there are) are walked.
 *   One wave per batch (k_vbg_group) finds every set's leader -- the lowest set of its batch that names the same entry --, numbers the batch's groups in leader
 *   order and gives every set the position lo_b + start_b[group] + rank, without atomics tickets; the blinded keys move to their positions and are summed per
 *   group; a Miller item takes H from the table and its key from the head of its range. A batch of more than MBLS_VBG_MAX_SETS sets is not grouped (each valid set
 *   is its own group: the verdict is the same). A batch whose groups reach beyond `bound` -- max_groups was too small -- is rejected with MBLS_ST_BAD_MSG_RANGE,
 *   its neighbours in front are untouched, nothing outside the call's workspace is read or written. _locate has no Miller value per set here: two shadow items per
 *   set and mbls_vsl.h's rule with the set's BATCH verdict in the place of the call's, both pairs' Miller loops in one launch, waves without a candidate idle.
 * HOST ENTRIES (_rng) draw exactly as mbls_verify_multiple_batches[_locate]_rng do. They refuse, with nothing queued and the outputs untouched, a batch table that
 *   is not sound and a committee id, key index or message index that names nothing; they count the groups themselves and take no max_groups.
 * n_batches = 0 and n_sets = 0 answer as mbls_verify_multiple_batches_device does.
 * PLANNING. mbls_plan_verify_multiple_batches_committee(limits, n_sets, n_batches, sets_per_batch (0: a ragged device-side table), table_size, max_groups, mode,
 *   locate, &plan), without a GPU: what a call reserves and acts on. MBLS_ERR_ARGUMENT for n_sets = 0, n_batches = 0, a mode outside 0..2, a uniform layout with
 *   n_batches x sets_per_batch != n_sets.
 * OUT OF SCOPE: the mbls_multi handle, wire keys. (Committee spans per set: mbls_verify_multiple_batches_committee_span_msgtable*, below. One batch per caller,
 *   coalesced into such calls: the verify_multiple stream, mbls_stream_create_vm_committee, above.) */
#define MBLS_VBG_MAX_SETS 1024u
typedef struct mbls_vm_batches_committee_plan {
    int32_t route;                 /* MBLS_VM_ROUTE_* */
    int32_t miller;                /* MBLS_PAIRING_WAVE, _LANES2 or _LANE: the form of the one-pair Miller loops, by miller_items */
    uint32_t tree_levels;          /* per set: levels of the per-batch trees; grouped: levels of the per-group key sums */
    uint32_t product_levels;       /* levels of the per-batch product trees (per set: over the sets; grouped: over the group items) */
    uint64_t bound;                /* the bound on the distinct (batch, entry) pairs */
    uint64_t miller_items;         /* per set: n_sets + n_batches; grouped: n_batches + bound */
    uint64_t workspace_items;      /* what the call reserves (mbls_ctx_reserve) */
} mbls_vm_batches_committee_plan;
int mbls_plan_verify_multiple_batches_committee(const mbls_limits* limits, uint64_t n_sets, uint64_t n_batches, uint32_t sets_per_batch, uint64_t table_size,
                                                uint64_t max_groups, int mode, int locate, mbls_vm_batches_committee_plan* out);
int mbls_verify_multiple_batches_committee_msgtable_device(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* d_sigs96, const uint32_t* d_cmt_idx,
                                                           const uint8_t* d_bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* d_msg_idx,
                                                           const uint64_t* d_rands, uint64_t n_sets, const uint32_t* d_batch_offsets, uint32_t sets_per_batch,
                                                           uint64_t n_batches, uint64_t max_groups, uint8_t* d_results, uint32_t* d_status, void* stream);
int mbls_verify_multiple_batches_committee_msgtable_locate_device(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* d_sigs96,
                                                                  const uint32_t* d_cmt_idx, const uint8_t* d_bits, uint32_t bits_stride, const mbls_msgtable* mt,
                                                                  const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n_sets,
                                                                  const uint32_t* d_batch_offsets, uint32_t sets_per_batch, uint64_t n_batches, uint64_t max_groups,
                                                                  uint8_t* d_results, uint32_t* d_status, uint8_t* d_set_results, uint32_t* d_set_status, void* stream);
int mbls_verify_multiple_batches_committee_msgtable_rng(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* sigs96, const uint32_t* cmt_idx,
                                                        const uint8_t* bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n_sets,
                                                        const uint32_t* batch_offsets, uint32_t sets_per_batch, uint64_t n_batches, uint8_t* results,
                                                        mbls_scalar_source draw, void* user);
int mbls_verify_multiple_batches_committee_msgtable_locate_rng(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* sigs96, const uint32_t* cmt_idx,
                                                               const uint8_t* bits, uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* msg_idx,
                                                               uint64_t n_sets, const uint32_t* batch_offsets, uint32_t sets_per_batch, uint64_t n_batches,
                                                               uint8_t* results, uint8_t* set_results, uint32_t* set_status, mbls_scalar_source draw, void* user);

/* MANY verify_multiple BATCHES PER CALL OVER COMMITTEE SPANS AND THE RESIDENT MESSAGE TABLE. Range sync and block import verify many blocks at once, each block
 * one verify_multiple batch of about a dozen sets, of which an attestation names up to 64 committees. These entries answer PER BATCH (per block), with per-set
 * location: the SETS are exactly those of mbls_verify_multiple_committee_span_msgtable[_locate]_device (`committees, d_sigs96, d_cmt_ids, n_cmt_ids, d_cmt_off,
 * d_bits, bits_stride, mt, d_msg_idx, d_rands, n_sets`), the BATCH TABLE AND OUTPUTS exactly those of mbls_verify_multiple_batches_committee_msgtable[_locate]_device
 * (`d_batch_offsets, sets_per_batch, n_batches, max_groups, d_results, d_status[, d_set_results, d_set_status], stream`). Every rule of "verify_multiple OVER
 * COMMITTEE SPANS" (the span rules, the single-key set, the per-segment route, malformed sets rejected on the device like a set that lists 0xFFFFFFFF) and every
 * rule of "MANY verify_multiple BATCHES PER CALL OVER COMMITTEE BITFIELDS" (a faulty device-side batch table, a max_groups that is too small, the
 * MBLS_VBG_MAX_SETS cap, n_batches = 0 and n_sets = 0, routing, enqueue only) holds unchanged and is not restated here.
 * A malformed set, or a message index at or above the table's size (MBLS_ST_BAD_MSG_RANGE), rejects ITS BATCH ONLY and is named by _locate.
 * CONTRACT. d_results[b], d_status[b], and for _locate every set byte and every set word, equal mbls_verify_multiple_batches[_locate]_indexed_device on the same
 *   signatures, scalars and batch table with every set's selected members spelled out in (segment, member) order and every message as the bytes of its entry, and
 *   equal one call of mbls_verify_multiple_committee_span_msgtable_locate_device per non-empty batch -- under every mode of mbls_ctx_set_vm_grouping and
 *   mbls_ctx_set_committee_route and every split factor. A set of one plain committee, and a single-key set, give what
 *   mbls_verify_multiple_batches_committee_msgtable_locate_device gives.
 * SPLIT. The factor P is the one-call entry's rule on the CALL's n_sets under mbls_ctx_set_vm_span_split; the 2 P n_sets partial sums stand in workspace items
 *   behind everything the batches plan lays out (csrc/mbls_vbg.h vbg_partial_first). The device work is the span key phase (k_vcs_expand, then the one-lane sum or
 *   k_vcs_partial_d / k_vcs_combine) followed by the batches entries' path: existing kernels launched from a new place, no kernel of its own.
 * HOST ENTRIES (_rng) draw exactly as mbls_verify_multiple_batches_committee_msgtable[_locate]_rng do. They refuse with MBLS_ERR_ARGUMENT, nothing queued and the
 *   outputs untouched, a batch table that is not sound, a malformed set, and a key or message index that names nothing; they count the groups themselves.
 * PLANNING. mbls_plan_verify_multiple_batches_committee_span(limits, n_sets, n_batches, sets_per_batch, table_size, max_groups, mode, locate, stride_words,
 *   split_mode, &plan, &split), without a GPU: plan holds the values of mbls_plan_verify_multiple_batches_committee for the same arguments with workspace_items
 *   raised by 2 P n_sets when P > 1; split is P (stride_words as in mbls_plan_verify_multiple_span). Argument errors: that function's, and a split_mode outside
 *   {0, 1, 2, 4, 8, 16}.
 * OUT OF SCOPE: a stream of span batches, the shared-list and per-set message forms, the mbls_multi handle and the shard form, wire keys, set kinds beyond span
 * and single key, splitting the chain of cached sums, a split factor per batch. */
int mbls_plan_verify_multiple_batches_committee_span(const mbls_limits* limits, uint64_t n_sets, uint64_t n_batches, uint32_t sets_per_batch, uint64_t table_size,
                                                     uint64_t max_groups, int mode, int locate, uint64_t stride_words, int split_mode,
                                                     mbls_vm_batches_committee_plan* out, uint32_t* split);
int mbls_verify_multiple_batches_committee_span_msgtable_device(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* d_sigs96, const uint32_t* d_cmt_ids,
                                                                uint64_t n_cmt_ids, const uint32_t* d_cmt_off, const uint8_t* d_bits, uint32_t bits_stride,
                                                                const mbls_msgtable* mt, const uint32_t* d_msg_idx, const uint64_t* d_rands, uint64_t n_sets,
                                                                const uint32_t* d_batch_offsets, uint32_t sets_per_batch, uint64_t n_batches, uint64_t max_groups,
                                                                uint8_t* d_results, uint32_t* d_status, void* stream);
int mbls_verify_multiple_batches_committee_span_msgtable_locate_device(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* d_sigs96,
                                                                       const uint32_t* d_cmt_ids, uint64_t n_cmt_ids, const uint32_t* d_cmt_off, const uint8_t* d_bits,
                                                                       uint32_t bits_stride, const mbls_msgtable* mt, const uint32_t* d_msg_idx,
                                                                       const uint64_t* d_rands, uint64_t n_sets, const uint32_t* d_batch_offsets,
                                                                       uint32_t sets_per_batch, uint64_t n_batches, uint64_t max_groups, uint8_t* d_results,
                                                                       uint32_t* d_status, uint8_t* d_set_results, uint32_t* d_set_status, void* stream);
int mbls_verify_multiple_batches_committee_span_msgtable_rng(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* sigs96, const uint32_t* cmt_ids,
                                                             uint64_t n_cmt_ids, const uint32_t* cmt_off, const uint8_t* bits, uint32_t bits_stride,
                                                             const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n_sets, const uint32_t* batch_offsets,
                                                             uint32_t sets_per_batch, uint64_t n_batches, uint8_t* results, mbls_scalar_source draw, void* user);
int mbls_verify_multiple_batches_committee_span_msgtable_locate_rng(mbls_ctx* ctx, const mbls_committees* committees, const uint8_t* sigs96, const uint32_t* cmt_ids,
                                                                    uint64_t n_cmt_ids, const uint32_t* cmt_off, const uint8_t* bits, uint32_t bits_stride,
                                                                    const mbls_msgtable* mt, const uint32_t* msg_idx, uint64_t n_sets, const uint32_t* batch_offsets,
                                                                    uint32_t sets_per_batch, uint64_t n_batches, uint8_t* results, uint8_t* set_results,
                                                                    uint32_t* set_status, mbls_scalar_source draw, void* user);
/* test probe: the grouping of the grouped route alone (set map, k_vbg_group, the scan of the group counts) on host buffers and ANY batch table, faulty ones
 * included. Arrays over the sets: n_sets words each (0xFFFFFFFF: none); group_count: n_batches; group_off: n_batches + 1. */
int mbls_vbg_group_probe(mbls_ctx* ctx, const uint32_t* msg_idx, uint64_t n_sets, uint64_t table_size, const uint32_t* batch_offsets, uint32_t sets_per_batch,
                         uint64_t n_batches, uint32_t* set_pos, uint32_t* set_status, uint32_t* pos_lo, uint32_t* pos_hi, uint32_t* group_head, uint32_t* group_entry,
                         uint32_t* group_count, uint32_t* group_off);

/* ---- batch helpers used to build inputs and caches on the device ---- */
/* n x PublicKey::from_bytes[_unchecked] / from_uncompressed_bytes: errs[i] = MBLS_OK / MBLS_ERR_* per key */
int mbls_pk_decode_batch(mbls_ctx* ctx, const uint8_t* in, int in_format, int validate, uint64_t n, uint8_t* out96, uint8_t* errs);
int mbls_pk_compress_batch(mbls_ctx* ctx, const uint8_t* in96, uint64_t n, uint8_t* out48, uint8_t* errs);
/* n x Signature::from_bytes: errs[i]; in_g2 (optional) = subgroup_check_g2 per signature */
int mbls_sig_check_batch(mbls_ctx* ctx, const uint8_t* in96, uint64_t n, uint8_t* errs, uint8_t* in_g2);
/* SECRET KEYS ON THE DEVICE (signing, sk -> pk; reference src/signature.rs:17-21, src/keys.rs:124-137 -- amcl's g1mul / g2mul select table entries in
 * constant time). Every table lookup that depends on a key is a SCAN WITH SELECTION: signing reads all eight records of the lane's window table in every
 * window and keeps its own with v_cndmask (the generated routine's constant-time form, tools/gen_tower_d.py blind_scan_ct), sk -> pk reads all 16 multiples
 * [d 16^j] G1 of every window and keeps record d_j (k_sk_select) -- no address, no instruction stream and no memory-operation count depends on a key; the
 * scalar's other uses (digit extraction, sign / zero handling) are selections as well. mbls_ctx_set_secret_ops(ctx, 1) (environment MBLS_UNSAFE_SECRET_OPS
 * for new contexts) switches both to the faster forms that read ONE record at a key-dependent address -- for building test and bench inputs from throw-away
 * keys only (measured at 2^16: signing 14.5 instead of 15.3 ms, sk -> pk 0.9 instead of 2.7 ms). This is NOT a claim of resistance against power or fault analysis, and a GPU shared with an attacker's kernels
 * is not a place for long-term keys either way.
 * WHAT THE CALLS LEAVE BEHIND (tests/test_gpu_secret_residue.py reads every device allocation of the context back -- mbls_ctx_residue_read below -- after the
 * same call on two key sets that differ in every digit, and holds the two images EQUAL but for the staged output; the list is what that test holds to zero).
 * Zeroed on the stream before the call's workspace is released, for the items of the largest chunk (which every chunk reuses):
 *   signing   workspace slots 3..6 (psi^j(H)), 25..30 (the partial products and their sums), 43..48 (the sum tree's parked operands), 49..102 (the window
 *             tables and the selected records) of items [0, 4 * chunk);
 *   sk -> pk  d_sksel (constant-time form: the selected multiples) or d_skidx (variable-time form: the keys' hexadecimal digits), workspace slots 0..2 (the
 *             key sum) and the status words of items [0, chunk) -- MBLS_ST_PK_INFINITY there marks a key with a digit 0;
 *   the host entries (mbls_sign_batch, mbls_sk_to_pk_batch, mbls_sign, mbls_pk_from_secret_key) besides: the staged keys, stage[0] bytes [0, 32 n), also when
 *             the device entry returns an error. Their staged OUTPUT -- stage[2] bytes [0, 96 n) / stage[1] bytes [0, 48 n or 96 n) -- stays until the next call.
 * Nothing else the context owns depends on the keys once the call's stream work is done. NOT claimed: LDS and registers after a kernel has ended (the spill
 * area of k_sign_blind and the tree levels, the accumulators of k_sk_select); memory the context has returned to the allocator with hipFree (a growing
 * workspace or staging buffer is freed as it is); a call that fails in the HIP runtime midway (the wipes are stream work like the rest); the caller's own
 * buffers of the device entries.
 * n x Signature::new / PublicKey::from_secret_key. Secret keys are NOT range-checked here: any 32-byte big-endian value gives [sk mod r] H(msg) /
 * [sk mod r] G1. The device entries use the context's workspace (four items per signature, in chunks of 65 536 signatures) and wait for its
 * previous user like the verification entries; they only enqueue. */
int mbls_sign_batch(mbls_ctx* ctx, const uint8_t* sks32, const uint8_t* msgs, uint32_t msg_len, uint64_t n, uint8_t* sigs96);
int mbls_sign_batch_device(mbls_ctx* ctx, const uint8_t* d_sks32, const uint8_t* d_msgs, uint32_t msg_len, uint64_t n, uint8_t* d_sigs96, void* stream);
int mbls_sk_to_pk_batch(mbls_ctx* ctx, const uint8_t* sks32, int out_format, uint64_t n, uint8_t* pks);
int mbls_sk_to_pk_batch_device(mbls_ctx* ctx, const uint8_t* d_sks32, int out_format, uint64_t n, uint8_t* d_pks, void* stream);
/* n x hash_to_curve_g2 (src/amcl_utils.rs:33-35), compressed output */
int mbls_hash_to_g2_batch(mbls_ctx* ctx, const uint8_t* msgs, uint32_t msg_len, uint64_t n, uint8_t* out96);
/* the same through the verification pipeline's own message phase, for the parity tests: mode 0 = the stand-alone lane body (as above),
 * 1 = the generated one-lane-per-item routine of the batch path, 2 = the one-wave-per-item program of small batches, 3 = two lanes per
 * message (the form batches between the wave engine's limit and half a round take) */
int mbls_hash_to_g2_batch_mode(mbls_ctx* ctx, const uint8_t* msgs, uint32_t msg_len, uint64_t n, uint8_t* out96, int mode);
/* test probe: everything of hash_to_curve_g2 AFTER hash_to_field. u192: n x (u0.c0, u0.c1, u1.c0, u1.c1), canonical
 * 48-byte big-endian values below p (MBLS_ERR_ARGUMENT otherwise). mode: 0 the compiled lane body, 1/2/3 as
 * mbls_hash_to_g2_batch_mode (generated lane routine / wave program / lane pair). out96: compressed H, infinity as 0xC0||0.. */
int mbls_map_to_g2_probe(mbls_ctx* ctx, const uint8_t* u192, uint64_t n, uint8_t* out96, int mode);
/* test probe: the Miller loop as a VALUE. in624: n x 13 canonical 48-byte big-endian values below p (MBLS_ERR_ARGUMENT otherwise) --
 * apk = G1 Jacobian X, Y, Z (Z = 0: infinity); sig = G2 affine x.c0, x.c1, y.c0, y.c1 (y = 0: infinity, as in the workspace); H = G2 Jacobian X.c0, X.c1,
 * Y.c0, Y.c1, Z.c0, Z.c1 (Z = 0: infinity). An import kernel puts them into workspace slots APK, SIG and H (mode 5: H into slot S), the form `mode` names
 * runs exactly what the pipeline launches for it, an export kernel writes out576: n x 12 coefficients in the order of slot F (c0.c0, c0.c1, c0.c2, c1.c0,
 * c1.c1, c1.c2 = the coefficients of w^0, w^2, w^4, w^1, w^3, w^5; real part first). With f(Q, P) = f_{|x|,Q}(P) CONJUGATED (x < 0), up to factors from
 * proper subfields of Fp12 (the projective formulas drop them; the final exponentiation kills them), a pair with an infinite member contributing 1:
 *   0  the compiled body (lane_miller without LDS)          f(sig, -G1) f(H, apk)
 *   1  k_miller, the generated two-pair routine             f(sig, -G1) f(H, apk)
 *   2  k_miller_single, the one-pair routine on one lane    f(H, apk)             (sig is not read)
 *   3  k_miller_single2, the same on a lane pair            f(H, apk)
 *   4  wave program miller1                                 f(H, apk)
 *   5  wave program smiller (S = H)                         conj(f(S, -G1))       (apk and sig are not read)
 * Modes 0..4 leave f itself in slot F -- "the conjugated values as k_miller_single leaves them" the n-pairing tails multiply --; mode 5 exports slots
 * 97..108, where smiller leaves the loop's value BEFORE the conjugation (vmfinal multiplies by its conjugate). Synchronises; host buffers. */
int mbls_miller_probe(mbls_ctx* ctx, const uint8_t* in624, uint64_t n, uint8_t* out576, int mode);
/* test probe: the final exponentiation as a VALUE. f576: n elements of Fp12, 12 canonical coefficients below p each in the order above, imported into
 * slot F. mode 0: the compiled final_exp (lane_final's fallback body), 1: k_final's generated routine (final_exp_ws_d), 2: k_final2's routine on a
 * lane pair (final_exp_ws_d2) -- kernels shaped like k_final / k_final2 (same launch bounds, same LDS array) that store f instead of folding it.
 * out576[i] = f_i^(3 (p^12 - 1) / r) (the CUBE of the usual value: see mbls_pairing.h), is_one[i] bit 0 = fp12_is_one of it as the kernel evaluates it;
 * mode 2: bit 1 of is_one[i] = the odd lane of item i came back with the even lane's value (compared on the device). mode 3: wave program vmfinal with
 * slot F = f_i and 1 in slots 97..108: a verdict only -- is_one[i], out576 is not written (and may be NULL). Synchronises; host buffers. */
int mbls_final_exp_probe(mbls_ctx* ctx, const uint8_t* f576, uint64_t n, uint8_t* out576, uint8_t* is_one, int mode);
/* n x AggregateSignature::aggregate (src/aggregates.rs:100-106): set i sums its k signatures (or the signatures
 * [offsets[i], offsets[i+1]) of sigs96), starting from infinity (an empty set gives 0xC0 || 0..). errs[i] = MBLS_OK or the
 * Signature::from_bytes error of the first member that does not decode. No subgroup check, like the reference. */
int mbls_aggregate_signatures_batch(mbls_ctx* ctx, const uint8_t* sigs96, const uint32_t* offsets, uint64_t n, uint32_t k, uint8_t* out96, uint8_t* errs);
int mbls_aggregate_signatures_batch_device(mbls_ctx* ctx, const uint8_t* d_sigs96, const uint32_t* d_offsets, uint64_t n_sets, uint32_t k,
                                           uint64_t total_sigs, uint8_t* d_out96, uint8_t* d_errs, void* stream);
/* n x AggregatePublicKey::aggregate over wire-format keys -> decoded aggregate keys */
int mbls_aggregate_public_keys_batch(mbls_ctx* ctx, const uint8_t* pks, int pk_format, const uint32_t* pk_offsets,
                                     uint64_t n, uint32_t k, uint8_t* apks96, uint32_t* status);
/* field probe for the parity tests of the hand-written routines, on canonical 48-byte big-endian values. op: 0 out = a*b,
 * 1 a^2, 2 Fp2 product and 3 Fp2 square over element pairs (2i, 2i+1) = (real, imaginary), 4 a^-1 (0 -> 0),
 * 5 a^((p-3)/4), 6 the paired-product routine on elements 2i and 2i+1 */
int mbls_fp_mul_batch(mbls_ctx* ctx, const uint8_t* a48, const uint8_t* b48, uint64_t n, uint8_t* out48, int op);
/* raw-register probe for the parity tests of the generated digit-form routines (tools/gen_tower_d.py probe_ops(): op = index in that list -- the eight
 * leaf bodies of tools/gen_fpd_asm.py, then the carry / reduce / pack / canonical passes and the word conversion). Lane i of n (at most 2^24) runs the body on the
 * int32 register contents in[w * n + i], w < n_in, and leaves the registers the probe lists in out[w * n + i], w < n_out; no value is interpreted or checked. MBLS_ERR_DEVICE if the library was built without the generated routines. */
int mbls_dform_probe_shape(int op, uint32_t* n_in, uint32_t* n_out);
int mbls_dform_probe(mbls_ctx* ctx, int op, const int32_t* in, uint64_t n, int32_t* out);
/* test probe: what a call LEFT in device memory (tests/test_gpu_secret_residue.py; "SECRET KEYS ON THE DEVICE" above). Reads only: no kernel is launched, no
 * secret is taken. mbls_ctx_residue_regions lists every device allocation the context owns: names[MBLS_RESIDUE_NAME_BYTES * i] (NUL-terminated) and bytes[i]
 * for region i < *n_regions, in an order that never changes -- "d_w" (the workspace: word-major, row 12 * slot + limb of *cap items of 4 bytes), "d_status",
 * "d_results", "d_scalar", "d_skidx", "d_sksel", the key staging, the shared-message and grouping tables, the committee and span scratches, "d_coop", "d_gtab",
 * then "stage[0]" .. the staging buffers of the host entries. A region that is not allocated yet has 0 bytes. names = bytes = NULL: the count alone;
 * max_regions below the count: MBLS_ERR_ARGUMENT. Key tables, message tables and committee tables are objects of their own and are not listed.
 * mbls_ctx_residue_read drains the device (hipDeviceSynchronize, under the context's lock) and copies [offset, offset + bytes) of region `region` to out. */
#define MBLS_RESIDUE_NAME_BYTES 16
int mbls_ctx_residue_regions(mbls_ctx* ctx, char* names, uint64_t* bytes, uint32_t max_regions, uint32_t* n_regions, uint64_t* cap);
int mbls_ctx_residue_read(mbls_ctx* ctx, uint32_t region, uint64_t offset, uint64_t bytes, uint8_t* out);
/* integer-ALU calibration: runs `iters` dependent Fp multiplications per lane on n lanes, returns elapsed ms */
int mbls_fp_mul_bench(mbls_ctx* ctx, uint64_t n_lanes, uint32_t iters, float* ms_out);

/* VALU issue-rate calibration for bench.py: every SIMD runs waves_per_simd (1..8) waves of `iters` x 128 instructions; mode 0:
 * v_mad_u64_u32, mode 1: v_add_co/v_addc chains. Returns elapsed ms (rate = waves_per_simd * iters * 128 / ms per SIMD).
 * mode 2: `iters` x 8 calls' worth of the generated Fp2 product routine inlined back to back (8 x 1 281 instructions per iteration, 980
 * multiply-accumulates each; use waves_per_simd <= 4): the rate of a kernel made of nothing but products. mode 3: the same with the paired
 * Fp product of the key-sum routines (8 x 923 instructions, 784 multiply-accumulates each). modes 4-6 (scripts/dbg/class_vs_mix.py): 8 multiply-accumulates + 4 plain
 * operations interleaved / in two blocks (192 instructions per iteration), the plain operations alone (128); mode 7: v_mad_i64_i32 on eight accumulators (128). */
int mbls_valu_bench(mbls_ctx* ctx, int mode, uint32_t waves_per_simd, uint32_t iters, float* ms_out);

/* ---- instrumentation: per-kernel HIP-event timing of the last *_device verify call (ms), for bench.py ---- */
#define MBLS_N_PHASES 6
int mbls_enable_phase_timing(mbls_ctx* ctx, int on);
int mbls_last_phase_ms(mbls_ctx* ctx, float ms[MBLS_N_PHASES]);   /* aggregate, sig, hash, miller, final, pack */

#ifdef __cplusplus
}
#endif
#endif

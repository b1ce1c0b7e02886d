/*
 * rsmi.h -- C ABI of the MI355X-native Reed-Solomon engine that replaces the
 * github.com/vivint/infectious calls on the shard encode/reconstruct path of
 * da-moon/noise-erasurecode-plugin.
 *
 * Every entry point names the reference call site it replaces.  The Go side
 * of the plugin (ShardPlugin, main.go:43-115/201-267) and the protobuf Shard
 * message (protobuf/shard.proto:21-27) stay unchanged; a cgo package exposing
 * NewFEC / (*FEC).Encode / (*FEC).Decode / Share on top of this header (see
 * INTEGRATION.md) is the only change the plugin needs (its import at
 * main.go:24).
 *
 * Conventions
 *  - k = MinimumNeededShards (data shards), n = TotalShards, m = n - k.
 *  - All arithmetic is GF(2^8), polynomial 0x11D, systematic Vandermonde code
 *    with evaluation points {0, 2^1, ..., 2^(n-1)} (infectious NewFEC).
 *  - Status codes are ints: RS_OK (0) or a negative rs_status.
 *  - Host pointers are never retained past a call (cgo rule).
 *  - Device pointers / streams are HIP device pointers / hipStream_t passed
 *    as void*; the stream may be NULL (legacy default stream).
 *  - An rs_ctx is bound to one HIP device (or to several: a device set,
 *    rs_new_devices below) and may be shared between threads
 *    (noise calls Receive concurrently, once per peer connection,
 *    main.go:49-52).  Each call leases its own stream, pinned staging and
 *    device workspace from a pool inside the ctx (RSMI_MAX_LEASES, default
 *    16, concurrent calls; more wait for a lease), so concurrent calls run
 *    concurrently.  The only shared state is the decode-pattern cache,
 *    guarded by a reader/writer lock: lookups and launches share it, only a
 *    call that meets a new erasure pattern takes it exclusively.
 *  - There is no CPU fallback: without a usable gfx950 device rs_new returns
 *    RS_EDEVICE.
 */
#ifndef RSMI_H
#define RSMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    RS_OK = 0,
    RS_EINVAL_KN = -1,         /* NewFEC: "requires 1 <= k <= n <= 256"            */
    RS_ELEN_NOT_MULTIPLE = -2, /* Encode: "input length must be a multiple of k"   */
    RS_ENOT_ENOUGH = -3,       /* Decode/Rebuild: NotEnoughShares                  */
    RS_EBAD_SHARE_ID = -4,     /* Rebuild: "invalid share id"                      */
    RS_ESINGULAR = -5,         /* invertMatrix: "singular matrix" (duplicate ids)  */
    RS_ENO_SHARES = -6,        /* Decode: "must specify at least one share"        */
    RS_ESHARE_LEN = -7,        /* shares of unequal length                         */
    RS_EINVAL = -8,            /* bad argument (NULL, misaligned device buffer...) */
    RS_EDEVICE = -9,           /* HIP runtime error or no gfx950 device            */
    RS_ENOMEM = -10,           /* host or device allocation failed                 */
    RS_ETOO_MANY_ERRORS = -16, /* Correct: TooManyErrors (Berlekamp-Welch failed)  */
} rs_status;

typedef struct rs_ctx rs_ctx;

/* ---- construction: replaces infectious.NewFEC(k, n) ---------------------
 * main.go:73 (receive side, k/n from the message) and main.go:248 (send
 * side, shardInput).  Builds the n x k systematic matrix once and uploads it;
 * the plugin re-creating a ctx per message is cheap but a cached ctx per
 * (k, n) is what INTEGRATION.md recommends. */
int rs_new(int k, int n, rs_ctx **out);                 /* current HIP device */
int rs_new_on_device(int k, int n, int device, rs_ctx **out);
void rs_free(rs_ctx *ctx);
int rs_k(const rs_ctx *ctx);
int rs_n(const rs_ctx *ctx);
int rs_device(const rs_ctx *ctx);
/* Copy of the n x k row-major encode matrix (infectious FEC.enc_matrix). */
int rs_encode_matrix(const rs_ctx *ctx, uint8_t *out);
const char *rs_strerror(int status);
/* Diagnostics: name of the kernel that serves encode (which = 0),
 * reconstruct (which = 1), verify (which = 2), update (which = 3), degraded
 * read (which = 4) or degraded check (which = 5) for this ctx, e.g.
 * "bitslice_k64_m16", "K10_MG4_B256", "verify_K10_MG4_B256",
 * "update_MG4_B256", "read_K10_MG4_B256" or "check_K10_MG4_B256"; which = 6:
 * the rs_combine variant that serves a narrow job of this code's shape (nsrc
 * = k, nout = min(m, 4), or 1 when m is 0), e.g. "combine_MG4_B256"; which =
 * 7: the rs_update_degraded variant, e.g. "update_degraded_MG4_B256" (no
 * reference counterpart); which = 8: the rs_correct_columns variant, e.g.
 * "columns_MG4_B256", or "none" for a code the call does not serve; which =
 * 9: the per-job-length twin of which = 6 that serves rs_combine_lens calls of
 * mixed lengths, e.g. "combine_lens_MG4_B256"; which = 10 and 11: the
 * pointer-mode twins of which = 5 and 8 that serve rs_verify_ptrs and
 * rs_correct_columns_ptrs, e.g. "check_K10_MG4_B256_ptrs" and
 * "columns_MG4_B256_ptrs"; which = 12 and 13: the repair kernel of
 * rs_reconstruct_checked and its pointer-mode twin of
 * rs_reconstruct_checked_ptrs, e.g. "repair_K10_MG4_B256" and
 * "repair_K10_MG4_B256_ptrs"; which = 14, 15 and 16: the per-stripe-length
 * twins of which = 2, 10 and 13 that serve rs_verify_ptrs_lens and
 * rs_reconstruct_checked_ptrs_lens calls of mixed lengths, e.g.
 * "verify_K10_MG4_B256_lens", "check_K10_MG4_B256_ptrs_lens" and
 * "repair_K10_MG4_B256_ptrs_lens"; which = 17: the per-job-length twin of
 * which = 11 that serves rs_correct_columns_ptrs_lens calls of mixed lengths,
 * e.g. "columns_MG4_B256_ptrs_lens" ("none" for m > 16); which = 18 and 19:
 * the sector-checksum kernel of the rs_crc32c_* calls and its pointer-mode
 * twin, "crc32c_H16_B256" and "crc32c_H16_B256_ptrs"; which = 20, 21 and 22:
 * the kernels that serve rs_encode_ptrs, rs_update_ptrs and rs_read_ptrs --
 * 20 is the name of which = 0 for a split-table code (that kernel reads the
 * table itself) and the generated pointer-mode twin for a bit-sliced one, e.g.
 * "bitslice_k64_m16_ptrs"; 21 and 22 are the pointer-mode twins of which = 3
 * and 4, e.g. "update_MG4_B256_ptrs" and "read_K10_MG4_B256_ptrs". */
const char *rs_kernel_name(const rs_ctx *ctx, int which);

/* ---- host-buffer API (the cgo path) -------------------------------------
 * rs_encode replaces (*FEC).Encode(input, output) at main.go:262.
 * input: len bytes, len % k == 0 (else RS_ELEN_NOT_MULTIPLE), S = len / k.
 * Data shares 0..k-1 are views input[i*S, (i+1)*S) (systematic, exactly as
 * infectious emits them); parity shares k..n-1 are written to
 * parity[(i-k)*S, (i-k+1)*S).  len == 0 is allowed (empty shares).
 * When input and parity are engine-pinned (rs_pinned_alloc / rs_arena),
 * 16-byte aligned with S % 16 == 0, and the code uses the split-table
 * kernel, the kernel reads and writes them in place over PCIe; rs_decode
 * likewise reads exactly k engine-pinned survivors in place (one launch, no
 * staging; dst written in place too when it is engine-pinned).  Pageable
 * buffers are staged through the lease's pinned memory, which the kernel
 * reads and writes over PCIe. */
int rs_encode(rs_ctx *ctx, const uint8_t *input, size_t len, uint8_t *parity);

/* rs_decode replaces (*FEC).Decode(dst, shares) at main.go:77: Correct, then
 * Rebuild.  numbers[count] / shares[count] describe the received
 * infectious.Share values; both arrays are sorted in place by number, like
 * infectious sorts the caller's slice.  Each share holds share_len bytes.
 * dst receives k * share_len bytes = the original input.
 * With exactly k distinct shares (the only case the plugin produces,
 * main.go:65) Correct has nothing to check.  With more, shares inconsistent
 * with one codeword are corrected by Berlekamp-Welch (up to
 * floor((count-k)/2) bad shares per byte column); the corrections go to dst
 * only -- unlike infectious, the caller's share bytes are not modified.
 * Errors: count < k -> RS_ENOT_ENOUGH; number outside [0, n) ->
 * RS_EBAD_SHARE_ID; fewer than k distinct numbers -> RS_ESINGULAR;
 * inconsistent shares with count - k < 2 -> RS_ENOT_ENOUGH; no codeword
 * within the correction radius -> RS_ETOO_MANY_ERRORS. */
int rs_decode(rs_ctx *ctx, int *numbers, const uint8_t **shares, int count,
              size_t share_len, uint8_t *dst);

/* rs_decode_batch: receive-side batching -- Decode
 * for `batch` messages of this code in one GPU pass.  Message b has
 * counts[b] shares; their numbers / pointers are consecutive in numbers[] /
 * shares[] (message b starts at sum(counts[0..b))), each share_len bytes;
 * dsts[b] receives k * share_len bytes.  Per-message results go to
 * status[b] (rs_decode's codes; each message's slice of numbers/shares is
 * sorted in place).  Messages with more than k distinct shares take the
 * rs_decode path (Correct); the rest are staged through pinned memory and
 * regenerated by rs_reconstruct_stripes launches that read the survivors over
 * PCIe where they lie (engine-pinned) or where they were staged, in chunks.
 * Batches beyond the pinned-staging cap (512 MiB; RSMI_BATCH_STAGE_MB) go in
 * groups of messages.  Returns RS_OK if every message decoded, else the first
 * failing status (in message order). */
int rs_decode_batch(rs_ctx *ctx, int batch, const int *counts, int *numbers,
                    const uint8_t **shares, size_t share_len, uint8_t **dsts, int *status);

/* rs_encode_batch: send-side batching, the counterpart of rs_decode_batch --
 * Encode (main.go:262, once per message in shardInput main.go:243-267) for
 * `batch` messages of this code in one GPU pass.  inputs[b] holds len bytes
 * (len % k == 0, else every status is RS_ELEN_NOT_MULTIPLE); parities[b]
 * receives (n - k) * len / k bytes laid out as rs_encode's parity.  The
 * messages are staged through pinned memory in chunks (the staging copy of
 * one chunk overlaps the kernel of the previous one, which reads and writes
 * the staging over PCIe), in groups of messages within the pinned-staging cap
 * (512 MiB; RSMI_BATCH_STAGE_MB).  status[b] gets each message's code;
 * returns RS_OK if every message encoded, else the first failing status. */
int rs_encode_batch(rs_ctx *ctx, int batch, const uint8_t *const *inputs, size_t len,
                    uint8_t *const *parities, int *status);

/* rs_encode_batch_lens / rs_decode_batch_lens: rs_encode_batch /
 * rs_decode_batch for messages of different lengths -- message b has
 * lens[b] input bytes / share_lens[b] bytes per share (HOST arrays of `batch`
 * entries, not retained), and everything else is as in those calls, message
 * by message: every message's output is bit-identical to what rs_encode /
 * rs_decode gives for it alone.  Real traffic does not come in equal lengths;
 * with these calls it is batched all the same.
 * Encode: lens[b] % k != 0 fails that message alone with
 * RS_ELEN_NOT_MULTIPLE, a NULL input or parity with a non-zero length fails
 * it alone with RS_EINVAL; a length of 0, or m == 0, is RS_OK with nothing
 * written.
 * Decode: validation, the in-place sort of each message's slice of numbers /
 * shares, the error codes and the Correct path (rs_decode) for messages with
 * more than k distinct shares are rs_decode_batch's; shares that alias any
 * message's dst are set aside first, each with its own length.
 * The GPU pass: the messages go in staging groups -- consecutive messages
 * while their staging (a slot of round_up(S_b, 64) bytes per shard) fits the
 * pinned-staging cap (512 MiB; RSMI_BATCH_STAGE_MB) -- and a group is one
 * pass of the per-job-length combine kernel (rs_combine_lens, rs_kernel_name
 * which = 9): message b is a job of k sources.  Encode's destinations are the
 * m parity rows, every job reading one shared copy of the encode matrix's
 * bottom rows; decode's are the message's erased DATA shards only, from the
 * k survivors in Rebuild's slot order (rs_pattern_survivors), with the decode
 * rows (those of rs_pattern_rows) built once per distinct erasure set of the
 * pass; present data shards are copied on the host while the GPU works, and a
 * message whose k survivors all lie 16-byte aligned in engine-pinned memory
 * is read in place (RS_STAT_BATCHES_IN_PLACE counts a pass whose messages all
 * are, RS_STAT_BATCHES_STAGED any other).  Within a group the messages go in
 * chunks cut at message boundaries and balanced by bytes: one chunk is staged
 * while the previous one is coded and the one before is copied out.
 * Pass-through: when all messages that are left to code have one length the
 * call is the equal-length call (same pass, same counters), which sends
 * exactly one message down the single-message path; a group of one message
 * -- one whose own staging exceeds the cap included -- takes that path too.
 * Device sets: contiguous message ranges, one per member, balanced by bytes.
 * status[b] gets each message's code; both return RS_OK if every message was
 * coded, else the first failing status in message order.  RS_EINVAL for a
 * NULL ctx (before any HIP call), batch < 0, or a NULL array with batch > 0. */
int rs_encode_batch_lens(rs_ctx *ctx, int batch, const uint8_t *const *inputs, const size_t *lens,
                         uint8_t *const *parities, int *status);
int rs_decode_batch_lens(rs_ctx *ctx, int batch, const int *counts, int *numbers, const uint8_t **shares,
                         const size_t *share_lens, uint8_t **dsts, int *status);

/* ---- device-resident batched API (many stripes per launch) ---------------
 * Stripe s, shard i lives at
 *     i <  k:  data   + s * data_stripe_stride   + i       * shard_pitch
 *     i >= k:  parity + s * parity_stripe_stride + (i - k) * shard_pitch
 * shard_len bytes are coded per shard; shard_pitch, both stripe strides and
 * both base pointers must be multiples of 16 and shard_pitch >=
 * round_up(shard_len, 16) (bytes between shard_len and the next multiple of
 * 16 are coded too: padding, never read back by the host API).
 *
 * rs_encode_stripes: parity of every stripe (stripe-batched (*FEC).Encode).
 * Enqueued on stream; returns when the launch is queued. */
int rs_encode_stripes(rs_ctx *ctx, const void *data, size_t data_stripe_stride,
                      void *parity, size_t parity_stripe_stride, size_t shard_pitch,
                      size_t shard_len, size_t stripes, void *stream);

/* rs_reconstruct_stripes: erased is a HOST array of stripes * n flags
 * (non-zero = shard i of stripe s is missing).  Every erased shard, data or
 * parity, is regenerated in place from k survivors chosen like infectious
 * Rebuild (data shares first, then the highest-numbered parity).  Per-pattern
 * decode matrices are inverted once and cached in the ctx.  A stripe with
 * more than m erasures -> RS_ENOT_ENOUGH (nothing is launched).  Enqueued on
 * stream (the small pattern tables are staged through pinned memory). */
int rs_reconstruct_stripes(rs_ctx *ctx, void *data, size_t data_stripe_stride,
                           void *parity, size_t parity_stripe_stride, size_t shard_pitch,
                           size_t shard_len, size_t stripes, const uint8_t *erased,
                           void *stream);

#define RS_VERIFY_CLEAN 0xFFFFFFFFu

/* Device-resident consistency check (the check half of infectious Correct,
 * stripe-batched).  Layout and argument rules as rs_encode_stripes.
 * first_bad: DEVICE array of `stripes` uint32, 4-byte aligned.
 * first_bad[s] = the lowest byte offset o < shard_len at which any stored
 * parity shard of stripe s differs from the parity recomputed from its k data
 * shards, or RS_VERIFY_CLEAN.
 * Reads data and parity only; writes nothing but first_bad.
 * Bytes at offsets >= shard_len (padding to 16, pitch gaps) are not compared.
 * Enqueued on stream; returns when queued. */
int rs_verify_stripes(rs_ctx *ctx, const void *data, size_t data_stripe_stride,
                      const void *parity, size_t parity_stripe_stride, size_t shard_pitch,
                      size_t shard_len, size_t stripes, uint32_t *first_bad, void *stream);

/* Scrub: verify, locate the corrupt shards of every inconsistent stripe,
 * regenerate them in place, verify again.
 * Repairs every stripe in which at most floor(m/2) shards (data or parity)
 * hold wrong bytes, however many bytes and wherever in those shards.
 * status (HOST, int[stripes], may be NULL): RS_OK or RS_ETOO_MANY_ERRORS per stripe.
 * rewritten (HOST, uint8_t[stripes*n], may be NULL): non-zero where shard i of
 * stripe s was regenerated.  For a stripe that ends RS_ETOO_MANY_ERRORS these
 * are the shards whose contents were replaced.
 * Synchronous: returns after the last verify has completed on stream.
 * Returns RS_OK if every stripe ends consistent, else RS_ETOO_MANY_ERRORS
 * (or an argument/device/memory error, in which case nothing is promised). */
int rs_correct_stripes(rs_ctx *ctx, void *data, size_t data_stripe_stride, void *parity,
                       size_t parity_stripe_stride, size_t shard_pitch, size_t shard_len,
                       size_t stripes, int *status, uint8_t *rewritten, void *stream);

/* Degraded scrub: the two calls above for stripes with missing shards.
 * Layout and alignment rules as rs_encode_stripes; erased is a HOST array of
 * stripes * n flags as for rs_reconstruct_stripes, not retained.  The slots
 * of erased shards are never dereferenced, for reading or writing.
 *
 * rs_verify_degraded: first_bad[s] (DEVICE, as for rs_verify_stripes) = the
 * lowest byte offset o < shard_len at which the PRESENT shards of stripe s do
 * not lie on one codeword, or RS_VERIFY_CLEAN.  For a stripe with e erasures
 * the k survivors Rebuild chooses recompute the other m - e present shards,
 * which are compared with the stored ones; the code is MDS, so the verdict
 * does not depend on that choice, and with e == 0 it is rs_verify_stripes'
 * (with no flag set at all the call is rs_verify_stripes).  A stripe with
 * exactly m erasures has no redundancy left: RS_VERIFY_CLEAN.  More than m
 * erasures in any stripe -> RS_ENOT_ENOUGH: nothing is launched and first_bad
 * is not written.  RS_EINVAL for NULL erased or first_bad and for what
 * rs_verify_stripes refuses, or stripes >= 2^32; stripes == 0 or
 * shard_len == 0: RS_OK.  Reads data and parity only; writes nothing but
 * first_bad.  A degraded stripe moves (k + m - e) * S bytes.  Enqueued on
 * stream; returns when queued (the small job tables are staged through pinned
 * memory).
 *
 * rs_correct_degraded: rs_correct_stripes with the erasures known from the
 * start.  Repairs every stripe with e erasures in which at most
 * floor((m - e) / 2) present shards hold wrong bytes, however many bytes and
 * wherever in those shards, by regenerating the located shards in place.  The
 * erased shards are NOT filled in (rs_reconstruct_stripes with the same flags
 * does that afterwards).  status and rewritten as for rs_correct_stripes;
 * rewritten is set for located shards only, never for erased ones.  An
 * inconsistent stripe with m - e < 2 ends RS_ETOO_MANY_ERRORS with nothing in
 * it written.  More than m erasures in any stripe -> RS_ENOT_ENOUGH: nothing
 * is launched or written.  Synchronous like rs_correct_stripes; with no flag
 * set it is rs_correct_stripes. */
int rs_verify_degraded(rs_ctx *ctx, const void *data, size_t data_stripe_stride,
                       const void *parity, size_t parity_stripe_stride, size_t shard_pitch,
                       size_t shard_len, size_t stripes, const uint8_t *erased,
                       uint32_t *first_bad, void *stream);
int rs_correct_degraded(rs_ctx *ctx, void *data, size_t data_stripe_stride, void *parity,
                        size_t parity_stripe_stride, size_t shard_pitch, size_t shard_len,
                        size_t stripes, const uint8_t *erased, int *status,
                        uint8_t *rewritten, void *stream);

/* Checked repair: rs_reconstruct_stripes that also says whether the survivors
 * it read could be trusted -- rs_verify_degraded and rs_reconstruct_stripes in
 * one pass over the stripe (n * S bytes moved per degraded stripe instead of
 * (2k + m) * S).  Layout, alignment, erased (HOST, stripes * n flags, not
 * retained) and first_bad (DEVICE, uint32[stripes]) as for rs_verify_degraded.
 * When stream has run:
 *  1. the slot of every erased shard holds the round_up(shard_len, 16) bytes
 *     rs_reconstruct_stripes would have written there, bit for bit, whether or
 *     not the stripe's check passes;
 *  2. first_bad[s] is what rs_verify_degraded would have written for the
 *     stripes as they were before the call: the lowest byte offset below
 *     shard_len at which the PRESENT shards of stripe s do not lie on one
 *     codeword, or RS_VERIFY_CLEAN.  Bytes at or beyond shard_len are not
 *     compared; a stripe with exactly m erasures has nothing to compare and is
 *     clean; a stripe without erasures gets rs_verify_stripes' verdict;
 *  3. nothing else is written: no present shard, no pad or pitch gap, no stride
 *     gap.  Of a stripe's present shards only Rebuild's k survivors and the
 *     m - e others that are compared are read, and nothing is ever read from
 *     the slot of an erased shard.
 * A stripe whose first_bad is not RS_VERIFY_CLEAN has had its missing slots
 * filled from survivors that cannot be trusted.  Keep that stripe's flags, run
 * rs_correct_columns (or rs_correct_degraded) with them, then reconstruct
 * again.
 * Refused with nothing launched or written: RS_ENOT_ENOUGH when any stripe has
 * more than m erasures; RS_EINVAL for a NULL ctx, NULL erased or first_bad, and
 * for everything rs_verify_degraded refuses (stripes >= 2^32 and the column
 * limit included).  stripes == 0 or shard_len == 0: RS_OK.  With m == 0 and no
 * flag set every stripe is clean.  Enqueued on stream; returns when queued,
 * like the two calls it fuses.  The stripes the repair kernel served count
 * into RS_STAT_REPAIR_CHECKED; stripes without erasures go through the verify
 * kernel and are not counted.  Two A/B knobs, both read at rs_new: a context
 * created under RSMI_REPAIR_FUSED=0 queues the two existing launches on stream
 * instead, with the same contract (its stripes count into
 * RS_STAT_CHECK_STRIPES and RS_STAT_REC_STRIPES_* as theirs do);
 * RSMI_XCD_REPAIR_REGION=N sets the repair kernel's blocks per XCD region (0:
 * natural order, the default for m <= 4; otherwise a stripe per region), as
 * RSMI_XCD_REC_REGION does for the reconstruct. */
int rs_reconstruct_checked(rs_ctx *ctx, void *data, size_t data_stripe_stride, void *parity,
                           size_t parity_stripe_stride, size_t shard_pitch, size_t shard_len,
                           size_t stripes, const uint8_t *erased, uint32_t *first_bad, void *stream);

/* Column scrub: infectious Correct, stripe-batched -- every byte column of
 * every stripe decoded on its own (Berlekamp-Welch's result, column by column).
 * Layout and alignment rules as rs_encode_stripes; erased (HOST, stripes * n
 * flags as for rs_reconstruct_stripes, not retained) may be NULL: nothing is
 * missing.  The slots of erased shards are never dereferenced.
 *
 * For stripe s and byte offset o < shard_len, with P the present shards of s,
 * r = |P| and y their r bytes at o:
 *  - y lies on a codeword of the code punctured to P: nothing is written;
 *  - else a codeword lies within Hamming distance floor((r - k) / 2) of y: it
 *    is unique, and exactly the bytes that differ from it are overwritten with
 *    its values;
 *  - else nothing in that column is written and stripe s ends
 *    RS_ETOO_MANY_ERRORS.  Beyond the radius the decoder may, like
 *    Berlekamp-Welch, land on another codeword.
 * The columns of a stripe do not depend on each other: a stripe with one
 * hopeless column still gets every other column repaired, and a later
 * rs_verify_stripes / rs_verify_degraded reports the first hopeless column as
 * first_bad.  So the call repairs any stripe in which each COLUMN has at most
 * floor((r - k) / 2) wrong shares, however many shards are touched overall --
 * three bad sectors on three devices at three offsets of an RS(10,4) stripe --
 * where rs_correct_stripes / rs_correct_degraded need at most that many wrong
 * SHARDS.  On scattered damage call it before or instead of them: the
 * shard-level scrub regenerates a located shard from survivors that may be
 * wrong at other columns, which spreads the damage.
 *
 * status (HOST, int[stripes], may be NULL): RS_OK or RS_ETOO_MANY_ERRORS.
 * corrected (HOST, uint32_t[stripes*n], may be NULL): corrected[s*n + i] = the
 * bytes of shard i of stripe s that the call changed; 0 for erased shards and
 * clean stripes.
 * Never read for comparison and never written: the slots of erased shards,
 * bytes at offsets >= shard_len (the pad to 16, pitch gaps), stride gaps,
 * clean stripes.  A wrong byte inside [shard_len, round_up(shard_len, 16)) is
 * not an error.
 * Refuses what rs_correct_degraded refuses, with the same codes: more than m
 * erasures in any stripe -> RS_ENOT_ENOUGH, nothing launched or written.  An
 * inconsistent stripe with r - k < 2 ends RS_ETOO_MANY_ERRORS unwritten; a
 * stripe with r == k is RS_OK.  stripes == 0, shard_len == 0 or m == 0: RS_OK.
 * Codes with m > 16 -> RS_EINVAL (the kernel keeps at most 16 syndromes per
 * column); every (k, n) with 1 <= m <= 16 is served, up to n = 256.
 * Synchronous like rs_correct_stripes: verify, one column launch over the
 * inconsistent stripes only (a call on clean stripes launches nothing more
 * than the verify), verify of those stripes again.  Returns RS_OK if every
 * stripe ends consistent, else RS_ETOO_MANY_ERRORS. */
int rs_correct_columns(rs_ctx *ctx, void *data, size_t data_stripe_stride, void *parity,
                       size_t parity_stripe_stride, size_t shard_pitch, size_t shard_len,
                       size_t stripes, const uint8_t *erased /* HOST, stripes*n, may be NULL */,
                       int *status /* HOST int[stripes], may be NULL */,
                       uint32_t *corrected /* HOST uint32[stripes*n], may be NULL */,
                       void *stream);

/* In-place parity update: overwrite data shards of stripes that already hold
 * parity and patch that parity from the difference alone.  Layout and
 * alignment rules as rs_encode_stripes.
 * updates: HOST array of `count` entries, not retained.  For each entry, data
 * shard `shard` of stripe `stripe` takes the contents at src (DEVICE, 16-byte
 * aligned, round_up(shard_len, 16) readable bytes, all of which are coded and
 * committed), and every parity shard r of that stripe becomes
 *     parity[r] ^= E[k + r][shard] * (old ^ new)
 * with E the encode matrix (rs_encode_matrix).  The stored parity is TRUSTED:
 * it is patched, not recomputed, so a stripe that was a codeword before the
 * call is one after it, and a stripe that was not (rs_verify_stripes) stays
 * inconsistent by the same difference.  Stripes and shards not listed are
 * neither read nor written; the other k - 1 data shards of an updated stripe
 * need not even be present.  Per stripe with j changed shards the call moves
 * (3j + 2m) * S bytes where copying the shards in and rs_encode_stripes moves
 * (2j + k + m) * S: it pays off while j + m < k, and the caller chooses.
 * A slice update -- bytes [o, o + l) of the shards, o a multiple of 16 -- is
 * the same call with data and parity advanced by o and shard_len = l (src then
 * holds the slice's new bytes); pitch and strides stay.
 * All or nothing: RS_EINVAL for NULL updates, stripe >= stripes, the same
 * (stripe, shard) listed twice, a NULL or misaligned src, a src range that
 * intersects the extent of the call's data or parity region, reserved != 0,
 * or more than 2^31 - 1 blocks; RS_EBAD_SHARE_ID for shard >= k; nothing is
 * launched then.  count == 0, stripes == 0 or shard_len == 0: RS_OK, nothing
 * launched.  With m == 0 only the data shards are overwritten.
 * Enqueued on stream; returns when queued (the small job tables are staged
 * through pinned memory). */
typedef struct rs_shard_update {
    uint64_t stripe;    /* < stripes */
    uint32_t shard;     /* data shard id, < k */
    uint32_t reserved;  /* 0 */
    const void *src;    /* DEVICE, 16-byte aligned, round_up(shard_len, 16) readable bytes */
} rs_shard_update;
int rs_update_stripes(rs_ctx *ctx, void *data, size_t data_stripe_stride, void *parity,
                      size_t parity_stripe_stride, size_t shard_pitch, size_t shard_len,
                      size_t stripes, const rs_shard_update *updates, size_t count,
                      void *stream);

/* In-place parity update of stripes with missing shards: rs_update_stripes
 * for a store that has lost shards and must go on accepting writes until the
 * repair has run.  Layout, alignment and `updates` as rs_update_stripes;
 * erased is a HOST array of stripes * n flags as for rs_reconstruct_stripes,
 * not retained; only the flags of listed stripes are examined.
 * For a listed stripe with erased set X (e ids, e_par of them parity) and
 * changed data shards U = U_p (present) + U_x (erased), every PRESENT parity
 * shard r becomes
 *     parity[r] ^= sum_{c in U} E[k + r][c] * (old_c ^ new_c).
 * For c in U_p old_c is read from the shard's slot, which then takes the new
 * contents.  For c in U_x old_c is regenerated from the k survivors Rebuild
 * chooses for X, read in their state before the call, with the decode row of
 * the ctx's pattern cache that rs_read_stripes would use (the row of c's rank
 * among the erased ids); the slot of c is NOT written: its new contents live
 * in the parity alone, and a later rs_reconstruct_stripes with the same flags
 * produces them.  The slots of erased shards, data or parity, changed or not,
 * are never dereferenced, for reading or writing.
 * Trust: the stored shards are patched, not recomputed.  A stripe whose
 * present shards lay on one codeword before the call (rs_verify_degraded)
 * still does after it.  A wrong byte in a present parity shard that is not
 * one of the survivors stays wrong by the same XOR difference, as for
 * rs_update_stripes; the survivors are trusted as the parity is: a wrong byte
 * in one of them goes into the regenerated old_c and from there into every
 * present parity shard.
 * Bytes moved per stripe with j changed shards (j_p of them present), S =
 * shard_len: with U_x empty (3j + 2(m - e_par)) * S; with U_x non-empty, on
 * the fused path, (k + j + j_p + 2(m - e_par)) * S in one pass and without
 * scratch -- the survivors are read instead of the old contents; that pass does
 * (m - e_par) * (k + j) multiplies per column, every source into every present
 * parity row, and is compute-bound for wide codes.  Where only
 * the changed shard is missing and the other k - 1 data shards are present,
 * copying nothing and re-encoding from the new contents costs (k + m - e_par)
 * * S and is cheaper; the caller chooses.
 * The fused path serves a call unless m > 16 or the tables of its widest job
 * (k + j sources) pass the 64 KiB of LDS; such a call takes the SLOW path: the
 * old contents of its erased changed shards are regenerated by the degraded
 * read's kernel into a scratch buffer of the ctx's, round_up(shard_len, 16)
 * bytes for each of them, every stripe is then patched from (old, new) pairs,
 * and the new contents of present shards are copied in by a pass behind that.
 * A slice update works as documented for rs_update_stripes.
 * All or nothing: everything rs_update_stripes refuses, with its codes, and
 * RS_EINVAL for NULL erased; RS_ENOT_ENOUGH for a listed stripe that has an
 * erased changed shard and more than m erasures (defects of the list are
 * reported first, the flags are looked at last); RS_ENOMEM if the slow path's
 * scratch cannot be had; nothing is launched or written then.  A listed stripe
 * with more than m erasures whose changed shards are all present is served:
 * its patch needs no decode.  count == 0, stripes == 0 or shard_len == 0:
 * RS_OK, nothing launched.  With m == 0 present changed shards are
 * overwritten and an erased one is RS_ENOT_ENOUGH.  If no listed stripe has a
 * flag set the call is rs_update_stripes.
 * Enqueued on stream; returns when queued (the small job tables are staged
 * through pinned memory). */
int rs_update_degraded(rs_ctx *ctx, void *data, size_t data_stripe_stride, void *parity,
                       size_t parity_stripe_stride, size_t shard_pitch, size_t shard_len,
                       size_t stripes, const uint8_t *erased,
                       const rs_shard_update *updates, size_t count, void *stream);

/* Degraded read: fetch listed shards of stripes while some of their shards
 * are missing, without repairing anything.  Layout and alignment rules as
 * rs_encode_stripes; erased is a HOST array of stripes * n flags as for
 * rs_reconstruct_stripes.
 * reads: HOST array of `count` entries, not retained.  For each entry, dst
 * receives the contents of shard `shard` (data or parity) of stripe `stripe`:
 * a shard that is not erased is copied; an erased one is computed from the k
 * survivors Rebuild chooses for the stripe's erasure set (data shares first,
 * then the highest-numbered parity) with the decode row of the ctx's pattern
 * cache that rs_reconstruct_stripes would use for it (row t of a pattern
 * regenerates the t-th erased id in increasing order, rs_pattern_rows).
 * round_up(shard_len, 16) bytes of dst are written; those past shard_len are
 * unspecified.
 * The data and parity regions are only read; the slots of erased shards are
 * never dereferenced, for reading or writing; stripes that are not listed are
 * not touched and their erased flags not examined.  Per stripe with j wanted
 * missing shards the call moves (k + j) * S bytes and does j * k multiplies
 * per column, where the repair of its e erasures moves (k + e) * S and does
 * e * k; wide codes are read with the split-table kernel too, never through
 * the syndrome network.
 * A slice read -- bytes [o, o + l) of the shards, o a multiple of 16 -- is
 * the same call with data and parity advanced by o and shard_len = l; pitch
 * and strides stay.
 * All or nothing: RS_EINVAL for NULL erased or reads, stripe >= stripes, the
 * same (stripe, shard) listed twice, a NULL or misaligned dst, reserved != 0,
 * a dst range that intersects the extent of the call's data or parity region
 * or another dst range, or more than 2^31 - 1 blocks; RS_EBAD_SHARE_ID for
 * shard >= n; RS_ENOT_ENOUGH for a listed stripe that wants an erased shard
 * and has more than m erasures (defects of the list are reported first);
 * nothing is launched and no dst is written then.  A listed stripe with more
 * than m erasures that wants present shards only is served.  count == 0,
 * stripes == 0 or shard_len == 0: RS_OK, nothing launched.  With k == n every
 * entry is a copy.
 * Enqueued on stream; returns when queued (the small job tables are staged
 * through pinned memory). */
typedef struct rs_shard_read {
    uint64_t stripe;    /* < stripes */
    uint32_t shard;     /* any shard id, < n (data or parity) */
    uint32_t reserved;  /* 0 */
    void *dst;          /* DEVICE, 16-byte aligned, round_up(shard_len, 16) writable bytes */
} rs_shard_read;
int rs_read_stripes(rs_ctx *ctx, const void *data, size_t data_stripe_stride,
                    const void *parity, size_t parity_stripe_stride, size_t shard_pitch,
                    size_t shard_len, size_t stripes, const uint8_t *erased,
                    const rs_shard_read *reads, size_t count, void *stream);

/* Caller-chosen GF(2^8) combinations of device buffers: the primitive under
 * the encode, reconstruct, update and read calls, with the coefficients, the
 * inputs and the outputs all named by the caller (no reference counterpart).
 * The ctx's (k, n) plays no part; the ctx supplies the device, the lease and
 * the stream, as it does for rs_blake2b_device.
 * jobs: HOST array of `count` jobs, not retained, and neither are the host
 * arrays a job points to.  Job b computes, for every output row r < nout,
 *     dst[r]  = sum_c coef[r * nsrc + c] * src[c]     (accumulate == 0)
 *     dst[r] ^= sum_c coef[r * nsrc + c] * src[c]     (accumulate == 1)
 * over buffers of `len` bytes, in the engine's field (polynomial 0x11D).
 * Coefficients 0 and 1 are ordinary values: an all-zero row zeroes its dst
 * when overwriting and leaves it as it was when accumulating.  All addresses
 * are DEVICE addresses, 16-byte aligned; round_up(len, 16) bytes of every src
 * are read and of every dst are written, those past len being unspecified (as
 * for rs_read_stripes).
 * Overlap rule: sources may repeat and may overlap each other freely, within
 * a job and across jobs; a dst range may meet neither a src range of any job
 * of the call nor another dst range of the call (jobs, and row groups of one
 * job, run in different blocks, and row groups re-read the sources).  Two
 * accumulations into one dst therefore take two calls on one stream.
 * Bytes moved: the kernel codes a job's outputs in row groups of MG = 4, 8 or
 * 16 rows (the smallest that holds the call's largest nout, 16 beyond; 8 when
 * the call's largest nsrc is above 199 and its largest nout above 8), each
 * group reading the sources once, so with G = ceil(nout / MG) a job moves
 *     (G * nsrc + nout * (1 + accumulate)) * len
 * bytes: a job of nout <= 16 reads its sources once.
 * Two uses: a holder of some survivors of a stripe multiplies
 * them by their columns of a decode row (rs_pattern_rows, rs_pattern_survivors)
 * into one partial buffer and the owner accumulates the partials; a data
 * holder turns old and new contents of a shard into the m parity deltas
 * E[k + r][shard] * (old ^ new) and the parity holder accumulates them with
 * coefficient 1.
 * All or nothing: RS_EINVAL for a NULL ctx (before any HIP call), NULL jobs
 * with count > 0, a job's src, dst or coef NULL, nsrc or nout outside 1..256,
 * accumulate > 1, reserved != 0, a NULL or misaligned address, a forbidden
 * overlap, count >= 2^32, a len the stripe calls refuse, tables of 2^32 or
 * more addresses or coefficients, or more than 2^31 - 1 blocks; nothing is
 * launched and nothing written then.  count == 0 or len == 0: RS_OK, nothing
 * launched.
 * Device sets: the call runs on the member on the device that holds
 * jobs[0].dst[0], RS_EINVAL if there is none; sources on a peer device are
 * read where they lie, as rs_reconstruct_spread does.
 * Enqueued on stream; returns when queued (the small tables are staged
 * through pinned memory). */
typedef struct rs_combine_job {
    const uint64_t *src;   /* HOST array of nsrc DEVICE addresses                */
    const uint64_t *dst;   /* HOST array of nout DEVICE addresses                */
    const uint8_t  *coef;  /* HOST, nout x nsrc row-major GF(2^8) coefficients   */
    uint32_t nsrc;         /* 1..256 */
    uint32_t nout;         /* 1..256 */
    uint32_t accumulate;   /* 0: dst[r] = sum_c coef[r][c]*src[c];  1: dst[r] ^= that sum */
    uint32_t reserved;     /* 0 */
} rs_combine_job;
int rs_combine(rs_ctx *ctx, const rs_combine_job *jobs, size_t count, size_t len, void *stream);

/* rs_combine_lens: rs_combine with a length per job -- `len` replaced by
 * lens[b] for job b, word for word.  lens: HOST array of `count` lengths, not
 * retained.  round_up(lens[b], 16) bytes of each of job b's sources are read
 * and of each of its destinations are written, and nothing past that; a store
 * that holds objects of different sizes codes them in one call where
 * rs_combine takes one call per distinct length.
 * A job with lens[b] == 0 is validated like any other (NULL arrays, nsrc and
 * nout ranges, reserved, addresses) but reads nothing, writes nothing, has no
 * ranges for the overlap rule and is not counted in RS_STAT_COMBINE_JOBS /
 * _ROWS.
 * Overlap rule: rs_combine's, each range as long as its own job's span: with
 * span_b = round_up(lens[b], 16), a dst range [d, d + span_b) of job b may
 * meet neither a src range [s, s + span_b') of any job b' nor another dst
 * range of the call.
 * Bytes moved: the row groups of MG rows are chosen once for the call, from
 * the largest nsrc and nout of the jobs that have bytes, as rs_combine does;
 * with G_b = ceil(nout_b / MG) job b moves
 *     (G_b * nsrc_b + nout_b * (1 + accumulate_b)) * lens[b]
 * bytes.
 * Kernel: jobs of different lengths run the per-job-length twin of the
 * combine kernel (rs_kernel_name which = 9), whose blocks find their job by a
 * search of a prefix sum of the jobs' block counts; the device tables grow
 * with the jobs, not with the bytes.  A call whose jobs all have one length is
 * rs_combine itself: same kernel (which = 6), same stats.
 * All or nothing: rs_combine's refusals, and RS_EINVAL for lens == NULL with
 * count > 0, any lens[b] of 2^28 or more 16-byte columns, or more than
 * 2^31 - 1 blocks in all.  count == 0 or every length 0: RS_OK, nothing
 * launched.
 * Device sets: the call runs on the member on the device that holds the first
 * destination of the first job with a non-zero length.
 * Enqueued on stream; returns when queued, as rs_combine. */
int rs_combine_lens(rs_ctx *ctx, const rs_combine_job *jobs, size_t count, const size_t *lens, void *stream);

/* rs_reconstruct_ptrs: rs_reconstruct_stripes with shards anywhere in
 * device memory.  shard_ptrs is a DEVICE array [stripes][n] of device
 * addresses (16-byte aligned): shard i of stripe s is read (survivor) or
 * written (erased) at shard_ptrs[s * n + i]; entries of present shards that
 * Rebuild does not choose are never dereferenced.  shard_len bytes per
 * shard (round_up(shard_len, 16) are coded).  The survivor gather of the
 * shard-distributed placement reconstructs straight out of its receive
 * buffers with it, and rs_decode_batch out of its packed
 * staging.  Enqueued on stream. */
int rs_reconstruct_ptrs(rs_ctx *ctx, const uint64_t *shard_ptrs, size_t shard_len, size_t stripes,
                        const uint8_t *erased, void *stream);

/* The scrub of the pointer placement: shard_ptrs as for rs_reconstruct_ptrs
 * (DEVICE, [stripes][n], 8-byte aligned, 16-byte-aligned addresses, only
 * read), and "the slot of shard i of stripe s" is shard_ptrs[s * n + i].
 * erased: HOST, stripes * n flags, non-zero = missing; NULL or no flag set =
 * every shard present.  Table entries of erased shards may hold anything and
 * are never dereferenced, for reading or writing;
 * round_up(shard_len, 16) bytes of every present shard of a checked stripe
 * are read.  Refused with nothing launched or written: RS_EINVAL for a NULL
 * or misaligned table (or first_bad), shard_len of 2^28 or more 16-byte
 * columns, stripes >= 2^32; RS_ENOT_ENOUGH when a stripe has more than m
 * erasures.  RS_OK for stripes == 0 or shard_len == 0, and for m == 0 (every
 * stripe RS_VERIFY_CLEAN).  Both count into RS_STAT_CHECK_STRIPES, the
 * second into RS_STAT_COLUMN_STRIPES / RS_STAT_COLUMN_BYTES.
 *
 * rs_verify_ptrs is rs_verify_degraded (rs_verify_stripes when no flag is
 * set) on that placement: first_bad (DEVICE, uint32[stripes]) and
 * RS_VERIFY_CLEAN as there, a stripe with exactly m erasures is clean.  It
 * only reads, so table entries may repeat.  Enqueued on stream; returns when
 * queued.
 *
 * rs_correct_columns_ptrs is rs_correct_columns on that placement: the same
 * per-column decoding within floor((r - k) / 2), status (HOST int[stripes])
 * and corrected (HOST uint32[stripes * n]) as there, the same sequence
 * (verify, one column launch over the inconsistent stripes, verify of those
 * again), synchronous, RS_EINVAL for m > 16.  Bytes at offsets >= shard_len,
 * clean stripes and the table are never written.  The caller guarantees
 * (not checked: the table lives on the device) that the ranges of the
 * present shards named by the table do not overlap each other.
 *
 * rs_reconstruct_checked_ptrs is rs_reconstruct_checked on that placement:
 * the slots of rs_reconstruct_ptrs, the verdicts of rs_verify_ptrs, points 1
 * to 3 and the recipe as there, and the table itself is never written.
 * erased must not be NULL.  Unlike rs_verify_ptrs, the call loads the table
 * entries of ERASED shards: they are the destinations, so they have to be
 * valid (16-byte aligned, round_up(shard_len, 16) writable bytes) and disjoint
 * from each other and from every present shard of the call.  Counts into
 * RS_STAT_REPAIR_CHECKED. */
int rs_verify_ptrs(rs_ctx *ctx, const uint64_t *shard_ptrs, size_t shard_len, size_t stripes,
                   const uint8_t *erased, uint32_t *first_bad, void *stream);
int rs_reconstruct_checked_ptrs(rs_ctx *ctx, const uint64_t *shard_ptrs, size_t shard_len, size_t stripes,
                                const uint8_t *erased, uint32_t *first_bad, void *stream);
int rs_correct_columns_ptrs(rs_ctx *ctx, const uint64_t *shard_ptrs, size_t shard_len, size_t stripes,
                            const uint8_t *erased, int *status, uint32_t *corrected, void *stream);

/* The first half of a store's life on the pointer placement: write parity for
 * new stripes, overwrite shards in place, serve reads while shards are
 * missing.  shard_ptrs as for rs_verify_ptrs (DEVICE, [stripes][n], 8-byte
 * aligned, 16-byte-aligned addresses), and "the slot of shard i of stripe s"
 * is shard_ptrs[s * n + i].  The table is only read, and only by kernels: the
 * host never copies it back, so a caller needs no host copy of it, and all
 * three calls are enqueued on stream and return when queued (the small job
 * tables are staged through pinned memory).  Safe from several threads on one
 * ctx; a device set routes by the table's device.
 * Refused by all three with nothing launched or written: RS_EINVAL for a NULL
 * ctx, a NULL or misaligned table, 2^28 or more 16-byte columns, stripes >=
 * 2^32, or more than 2^31 - 1 blocks.  RS_OK with nothing launched for
 * stripes == 0 or shard_len == 0, and count == 0 where there is a list.
 * The caller guarantees what the host cannot check, because the table lives
 * on the device: the ranges of the slots a call touches do not overlap each
 * other (as for rs_correct_columns_ptrs), and no src or dst range meets one.
 *
 * rs_encode_ptrs is rs_encode_stripes on that placement: parity shard r of
 * stripe s is written at shard_ptrs[s * n + k + r], and its round_up(shard_len,
 * 16) bytes are bit for bit what rs_encode_stripes writes for the same data.
 * The k data shards of every stripe are only read and nothing else is written;
 * a stripe moves (k + m) * S bytes.  The kernel is the one that serves
 * rs_encode_stripes for the code: the split-table kernel reading the table, or
 * the generated twin of the bit-sliced network (rs_kernel_name which = 20).
 * m == 0: RS_OK.  No lock and no lease, as rs_encode_stripes.
 *
 * rs_update_ptrs is rs_update_stripes on that placement, for stripes without
 * missing shards: `updates` and its validation are those of rs_update_stripes
 * (RS_EINVAL for NULL updates, stripe >= stripes, a duplicate (stripe, shard),
 * a NULL or misaligned src, reserved != 0; RS_EBAD_SHARE_ID for shard >= k),
 * except that a src range cannot be checked against the slots.  For each entry
 * the slot of data shard `shard` of stripe `stripe` takes the contents at src,
 * and every parity shard r of that stripe becomes
 *     parity[r] ^= E[k + r][shard] * (old ^ new);
 * a stripe with j changed shards moves (3j + 2m) * S bytes.  Only the table
 * entries of a listed stripe's changed shards and of its m parity shards are
 * loaded: every other entry -- the stripe's other data shards, every entry of
 * an unlisted stripe -- is never dereferenced and may hold anything.  With
 * m == 0 only the data is overwritten.
 * Slices: the call works on bytes [shard_offset, shard_offset + shard_len) of
 * every slot it touches, and src holds the slice's new bytes from its start
 * (rs_update_stripes advances data and parity instead; a table cannot be
 * advanced without a second table).  shard_offset is a multiple of 16 and
 * shard_offset / 16 plus the column count stays below 2^28, else RS_EINVAL.
 * There is no pointer form of rs_update_degraded.  A stripe with an erased
 * changed shard takes two passes: rs_read_ptrs regenerates the old contents
 * into scratch (no host copy of the table needed for that half), then
 * rs_combine applies the deltas to the present parity, whose addresses the
 * caller names (DESIGN.md 4.15 measured that route at 0.78 / 0.77 of the HBM
 * peak where the fused strided kernel runs at 0.58 / 0.25).
 *
 * rs_read_ptrs is rs_read_stripes on that placement: erased (HOST, stripes * n
 * flags, not NULL), `reads` and its validation are those of rs_read_stripes
 * (RS_EINVAL for NULL erased or reads, stripe >= stripes, a duplicate (stripe,
 * shard), a NULL or misaligned dst, reserved != 0, two dst ranges that meet;
 * RS_EBAD_SHARE_ID for shard >= n; RS_ENOT_ENOUGH for a listed stripe that
 * wants an erased shard and has more than m erasures; a listed stripe with
 * more than m erasures that wants present shards only is served), except that
 * a dst range cannot be checked against the slots.  A present wanted shard is
 * copied; an erased one is computed from the k survivors Rebuild chooses, with
 * the row of the shared pattern cache; a stripe with j wanted missing shards
 * moves (k + j) * S bytes.  Nothing named by the table is written, and the
 * table entries of erased shards are never loaded.  shard_offset as for
 * rs_update_ptrs: bytes [shard_offset, shard_offset + shard_len) of the slots
 * are read and dst receives the slice from its start. */
int rs_encode_ptrs(rs_ctx *ctx, const uint64_t *shard_ptrs, size_t shard_len, size_t stripes, void *stream);
int rs_update_ptrs(rs_ctx *ctx, const uint64_t *shard_ptrs, size_t shard_offset, size_t shard_len, size_t stripes,
                   const rs_shard_update *updates, size_t count, void *stream);
int rs_read_ptrs(rs_ctx *ctx, const uint64_t *shard_ptrs, size_t shard_offset, size_t shard_len, size_t stripes,
                 const uint8_t *erased, const rs_shard_read *reads, size_t count, void *stream);

/* rs_verify_ptrs and rs_reconstruct_checked_ptrs for stripes that each have a
 * shard length of their own (a store of objects of different sizes, scrubbed
 * or repaired in one call): shard_lens is a HOST array of `stripes` lengths
 * and is not retained; everything else is as in the equal-length calls.
 * Stripe s is treated exactly as the equal-length call would treat it if it
 * were called on that stripe alone with shard_len = shard_lens[s]:
 *  - first_bad[s] is the lowest byte offset below shard_lens[s] at which the
 *    present shards of stripe s do not lie on one codeword, or
 *    RS_VERIFY_CLEAN; bytes at or beyond shard_lens[s] are never compared; a
 *    stripe with exactly m erasures is clean; erased == NULL (nothing missing)
 *    is allowed for the verify call only;
 *  - the repair call stores, in the slot of every erased shard of stripe s,
 *    the round_up(shard_lens[s], 16) bytes rs_reconstruct_ptrs would write
 *    there, whether or not the stripe's check passes, and writes nothing else:
 *    no present shard, nothing past round_up(shard_lens[s], 16) of any slot,
 *    never the table.  The verify call never loads the table entries of erased
 *    shards; for the repair call they are the destinations, valid and disjoint
 *    as for rs_reconstruct_checked_ptrs;
 *  - at most round_up(shard_lens[s], 16) bytes of a shard of stripe s are
 *    read, and a stripe moves the bytes of the equal-length call at its own
 *    length (stripes without erasures go through the verify kernel whatever m
 *    is);
 *  - a stripe with shard_lens[s] == 0 has its flags validated like any other
 *    (more than m erasures refuses the call); it reads nothing, writes nothing,
 *    gets RS_VERIFY_CLEAN and is counted in no stat.
 * Refused with nothing launched or written (first_bad included): RS_EINVAL
 * for a NULL ctx, NULL shard_lens with stripes > 0, everything the equal-length
 * call refuses (NULL or misaligned table or first_bad, stripes >= 2^32, NULL
 * erased for the repair), any length of 2^28 or more 16-byte columns, more
 * than 2^31 - 1 blocks in all (a block is 256 columns of a stripe for one row
 * group); RS_ENOT_ENOUGH when any stripe has more than m erasures.  RS_OK with
 * nothing written for stripes == 0 or when every length is 0; m == 0: every
 * stripe clean.
 * When every stripe has the same non-zero length the call IS the equal-length
 * call: same kernels, same stats (RSMI_SCRUB_LENS_FORCE=1, read once, for
 * measurements only, keeps such a call on the per-stripe-length kernels).
 * Otherwise compile-time twins of the verify, check and repair kernels
 * (rs_kernel_name which = 14, 15, 16) serve it, whose blocks find their stripe
 * by a search of a prefix sum of block counts; such a call counts one into
 * RS_STAT_SCRUB_LENS_LAUNCHES and its degraded stripes that have bytes into
 * RS_STAT_CHECK_STRIPES / RS_STAT_REPAIR_CHECKED, as the equal-length calls
 * do.  RSMI_REPAIR_FUSED=0 does not apply to the mixed-length repair: there is
 * no mixed-length unfused reconstruct, so it always runs the repair kernel's
 * twin.  Enqueued on stream; returns when queued; safe from several threads on
 * one ctx. */
int rs_verify_ptrs_lens(rs_ctx *ctx, const uint64_t *shard_ptrs, const size_t *shard_lens, size_t stripes,
                        const uint8_t *erased, uint32_t *first_bad, void *stream);
int rs_reconstruct_checked_ptrs_lens(rs_ctx *ctx, const uint64_t *shard_ptrs, const size_t *shard_lens,
                                     size_t stripes, const uint8_t *erased, uint32_t *first_bad, void *stream);

/* rs_correct_columns_ptrs for stripes that each have a shard length of their
 * own: the middle step of the recipe above for a store of objects of different
 * sizes, in one call.  shard_ptrs, erased, status and corrected are those of
 * rs_correct_columns_ptrs; shard_lens is a HOST array of `stripes` lengths and
 * is not retained.  Stripe s is treated exactly as rs_correct_columns_ptrs
 * would treat it if it were called on that stripe alone with shard_len =
 * shard_lens[s]:
 *  - every byte column o < shard_lens[s] is decoded on its own, within
 *    floor((r - k) / 2) of the r present shares; status[s] (HOST int[stripes],
 *    may be NULL) and corrected[s * n + i] (HOST uint32[stripes * n], may be
 *    NULL) mean what they mean there: RS_OK or RS_ETOO_MANY_ERRORS (a column
 *    beyond the radius, which is left alone while the others are corrected, or
 *    an inconsistent stripe with r - k < 2, which is not written at all), and
 *    the bytes changed in shard i; the call returns RS_ETOO_MANY_ERRORS when
 *    any stripe failed;
 *  - the same sequence: verify, one column launch over the inconsistent
 *    stripes only, verify of those stripes again; synchronous, two host round
 *    trips;
 *  - at most round_up(shard_lens[s], 16) bytes of a present shard of stripe s
 *    are read;
 *  - bytes at or beyond shard_lens[s] are never decoded and never written, so a
 *    wrong byte in [shard_lens[s], round_up(shard_lens[s], 16)) is not an error
 *    (padding a short object to a longer length is therefore no substitute:
 *    the bytes behind its length are no part of a codeword);
 *  - clean stripes are never written, table entries of erased shards are never
 *    loaded, the table itself is never written; the ranges of the present
 *    shards must not overlap (not checked);
 *  - a stripe with shard_lens[s] == 0 has its flags validated like any other;
 *    it reads nothing, writes nothing, ends RS_OK with zero corrected and is
 *    counted in no stat.
 * Refused with nothing launched and nothing written (status and corrected
 * included): RS_EINVAL for a NULL ctx (before any HIP call), NULL shard_lens
 * with stripes > 0, a NULL or misaligned table, stripes >= 2^32, any length of
 * 2^28 or more 16-byte columns, m > 16, more than 2^31 - 1 blocks in either
 * verify launch (rs_verify_ptrs_lens' bound), or more than 2^31 - 1 blocks in
 * the worst-case column launch, the sum over the stripes that have bytes of
 * ceil(ncols_s / 256) with ncols_s = round_up(shard_lens[s], 16) / 16 -- checked
 * up front, so the refusal does not depend on which stripes turn out
 * inconsistent; RS_ENOT_ENOUGH when any stripe, with or without bytes, has more
 * than m erasures.  RS_OK for stripes == 0; RS_OK with status all RS_OK and
 * corrected all 0 when every length is 0 or m == 0.
 * When every stripe has the same non-zero length the call IS
 * rs_correct_columns_ptrs: it calls it, same kernels, same stats
 * (RSMI_COLUMN_LENS_FORCE=1, read once, for measurements only, keeps such a
 * call on the twin).  Otherwise both verifies are rs_verify_ptrs_lens' launches
 * and count into RS_STAT_CHECK_STRIPES / RS_STAT_SCRUB_LENS_LAUNCHES exactly as
 * those calls would (the second is planned over the inconsistent stripes only),
 * and the column launch runs the per-job-length twin of the pointer-mode column
 * kernel (rs_kernel_name which = 17), whose blocks find their stripe by a
 * search of a prefix sum of block counts; it counts one into
 * RS_STAT_COLUMN_LENS_LAUNCHES, its stripes into RS_STAT_COLUMN_STRIPES and the
 * bytes it changed into RS_STAT_COLUMN_BYTES.  Safe from several threads on one
 * ctx. */
int rs_correct_columns_ptrs_lens(rs_ctx *ctx, const uint64_t *shard_ptrs, const size_t *shard_lens,
                                 size_t stripes, const uint8_t *erased /* HOST, may be NULL */,
                                 int *status /* HOST int[stripes], may be NULL */,
                                 uint32_t *corrected /* HOST uint32[stripes*n], may be NULL */,
                                 void *stream);

/* ---- sector checksums: CRC-32C of stored shards ----------------------------
 * Every scrub above asks whether the stored shards lie on a codeword.  These
 * calls ask what a store has to ask first -- are these the bytes that were
 * written? -- with a checksum per sector that is kept apart from the data.  A
 * mismatch LOCATES the damage, so errors become erasures: rs_correct_crc32c
 * repairs up to m wrong shards per stripe where the codeword scrubs repair
 * floor(m / 2), never lands on a wrong codeword, and catches what no codeword
 * check can: a valid codeword of the wrong data (a stale shard set, a lost
 * update).
 *
 * The checksum is CRC-32C (Castagnoli) exactly as iSCSI / RFC 3720 defines it:
 * reflected polynomial 0x82F63B78, initial value 0xFFFFFFFF, final XOR
 * 0xFFFFFFFF, stored as a host-order uint32_t ("123456789" -> 0xE3069283, the
 * empty message -> 0).  A shard of shard_len bytes has nsec = ceil(shard_len /
 * sector_len) sectors; the checksum of sector j covers the bytes [j *
 * sector_len, min((j + 1) * sector_len, shard_len)) and nothing else -- never
 * the padding up to 16 or the pitch gap -- so a host reproduces it from the
 * shard's contents alone (rs_crc32c_host).  sector_len is a power of two,
 * 512 <= sector_len <= 65536.
 *
 * Layout and alignment rules are those of rs_encode_stripes.  erased is a HOST
 * array of stripes * n flags as for rs_reconstruct_stripes, not retained; it
 * may be NULL (nothing missing) in every one of these calls.  The slots
 * of erased shards are never dereferenced, and in the pointer calls their
 * table entries are not loaded.  crcs is a DEVICE array of uint32_t, 4-byte
 * aligned: sector j of shard i of stripe s is crcs[(s * n + i) * crc_pitch +
 * j], crc_pitch >= nsec; entries between nsec and crc_pitch are never read or
 * written.  A slice call -- data and parity advanced by a multiple of
 * sector_len, crcs by the same number of sectors, shard_len shortened -- works
 * on a store's full table directly, as the slice forms of update and read do;
 * sector indices are then relative to the slice.  That is also the recipe for
 * sector-granular regeneration, which these calls do not do themselves: check,
 * then rs_read_stripes the slice that covers the bad sectors into place.
 *
 * rs_crc32c_stripes computes and stores the checksums of every present shard;
 * the entries of erased shards are left as they are.  Reads data and parity
 * only.  Enqueued on stream; returns when queued.
 *
 * rs_crc32c_check_stripes compares instead: first_bad (DEVICE,
 * uint32[stripes * n], 4-byte aligned) gets, at [s * n + i], the lowest sector
 * index of shard i of stripe s whose bytes do not match the stored checksum,
 * or RS_VERIFY_CLEAN; an erased shard gets RS_VERIFY_CLEAN.  Writes nothing
 * but first_bad.  Enqueued.  Copied to the host and reduced to non-zero / zero
 * (clean), it is an `erased` array for rs_reconstruct_stripes /
 * rs_reconstruct_checked.
 *
 * rs_crc32c_ptrs / rs_crc32c_check_ptrs are the same two calls for the pointer
 * placement of rs_reconstruct_ptrs (shard_ptrs: DEVICE, [stripes][n], 8-byte
 * aligned, 16-byte-aligned addresses, only read).
 *
 * rs_correct_crc32c is the repair, synchronous and shaped like
 * rs_correct_degraded:
 *  1. every present shard is checked; B(s) is the set of present shards of
 *     stripe s with a mismatching sector, X(s) its erased shards;
 *  2. B empty: the stripe is RS_OK and untouched (a clean stripe with more
 *     than m erasures too);
 *  3. |X + B| > m: the stripe is RS_ETOO_MANY_ERRORS and nothing in it is
 *     written;
 *  4. otherwise every shard of B is regenerated in place, whole, from the k
 *     survivors Rebuild chooses for X + B (the read path of rs_read_stripes:
 *     flags X + B, wanted B, every destination the shard's own slot; the slots
 *     of X are neither read nor written), all stripes in one batched launch;
 *  5. the regenerated shards are checked against their stored checksums again,
 *     in one launch over those shards only; one that still mismatches makes its
 *     stripe RS_ETOO_MANY_ERRORS: either its stored checksum is wrong, or a
 *     survivor is wrong under a matching checksum.
 * status (HOST int[stripes], may be NULL) and rewritten (HOST
 * uint8_t[stripes * n], may be NULL) as for rs_correct_degraded: rewritten is
 * non-zero for regenerated shards, never for erased ones.  Returns RS_OK if
 * every stripe ends with all present shards matching, else
 * RS_ETOO_MANY_ERRORS.  RS_ENOT_ENOUGH, with nothing written, when a stripe
 * with more than m erasures also has a mismatch.  Checksums are never written
 * by this call, and it does not ask whether a stripe is a codeword:
 * rs_verify_degraded answers that.  With m == 0 any mismatch is
 * RS_ETOO_MANY_ERRORS.
 *
 * All or nothing, before anything is launched: RS_EINVAL for a NULL ctx (before
 * any HIP call), NULL or misaligned crcs or first_bad, a sector_len that is not
 * a power of two in range, crc_pitch < nsec, stripes * n >= 2^32, more than
 * 2^31 - 1 blocks (a block is 64 KiB of a shard, or four sectors if that is
 * more), and whatever rs_verify_stripes / rs_verify_ptrs refuses.  stripes == 0
 * or shard_len == 0: RS_OK, nothing launched.  Device sets route by pointer as
 * rs_verify_stripes does.  RS_STAT_CRC_SECTORS counts the sectors checksummed
 * by any launch of these calls (the second check of rs_correct_crc32c
 * included), RS_STAT_CRC_REGENERATED the shards rs_correct_crc32c regenerated.
 * rs_kernel_name which = 18 and 19 name the kernel and its pointer twin. */
int rs_crc32c_stripes(rs_ctx *ctx, const void *data, size_t data_stripe_stride, const void *parity,
                      size_t parity_stripe_stride, size_t shard_pitch, size_t shard_len, size_t stripes,
                      const uint8_t *erased /* HOST, may be NULL */, size_t sector_len, uint32_t *crcs,
                      size_t crc_pitch, void *stream);
int rs_crc32c_check_stripes(rs_ctx *ctx, const void *data, size_t data_stripe_stride, const void *parity,
                            size_t parity_stripe_stride, size_t shard_pitch, size_t shard_len, size_t stripes,
                            const uint8_t *erased /* HOST, may be NULL */, size_t sector_len,
                            const uint32_t *crcs, size_t crc_pitch, uint32_t *first_bad, void *stream);
int rs_crc32c_ptrs(rs_ctx *ctx, const uint64_t *shard_ptrs, size_t shard_len, size_t stripes,
                   const uint8_t *erased /* HOST, may be NULL */, size_t sector_len, uint32_t *crcs,
                   size_t crc_pitch, void *stream);
int rs_crc32c_check_ptrs(rs_ctx *ctx, const uint64_t *shard_ptrs, size_t shard_len, size_t stripes,
                         const uint8_t *erased /* HOST, may be NULL */, size_t sector_len, const uint32_t *crcs,
                         size_t crc_pitch, uint32_t *first_bad, void *stream);
int rs_correct_crc32c(rs_ctx *ctx, void *data, size_t data_stripe_stride, void *parity,
                      size_t parity_stripe_stride, size_t shard_pitch, size_t shard_len, size_t stripes,
                      const uint8_t *erased /* HOST, may be NULL */, size_t sector_len, const uint32_t *crcs,
                      size_t crc_pitch, int *status /* HOST int[stripes], may be NULL */,
                      uint8_t *rewritten /* HOST uint8_t[stripes*n], may be NULL */, void *stream);
/* rs_crc32c_host: the host reference (slice-by-8): out[i] = CRC-32C of the
 * lens[i] bytes at bufs[i].  Needs no context and no GPU.  count == 0: RS_OK;
 * RS_EINVAL for count < 0, a NULL array with count > 0, or a NULL buffer of
 * non-zero length. */
int rs_crc32c_host(int count, const uint8_t *const *bufs, const size_t *lens, uint32_t *out);

/* Cached decode patterns held by the ctx (diagnostics / tests).  The cache
 * holds at most 2^20 patterns (RSMI_PATTERN_CAP); a call that would exceed
 * that evicts it whole, with no host synchronisation (the rebuilt rows wait
 * on the device for the launches that read the old ones).
 * rs_pattern_evictions counts those evictions. */
int rs_pattern_count(const rs_ctx *ctx);
int64_t rs_pattern_evictions(const rs_ctx *ctx);

/* Counters of a ctx (diagnostics / tests). */
enum {
    RS_STAT_PATTERNS = 0,          /* cached decode patterns                          */
    RS_STAT_EVICTIONS = 1,         /* pattern-cache evictions                         */
    RS_STAT_BATCHES_IN_PLACE = 2,  /* rs_decode_batch calls that read survivors in place */
    RS_STAT_BATCHES_STAGED = 3,    /* ... that staged them through pinned copies      */
    RS_STAT_LEASES = 4,            /* leases created (peak concurrent calls)          */
    RS_STAT_ENCODES_IN_PLACE = 5,  /* rs_encode calls served from engine-pinned memory */
    RS_STAT_DECODES_IN_PLACE = 6,  /* rs_decode calls that read engine-pinned survivors in place */
    RS_STAT_REC_STRIPES_TABLE = 7,  /* stripes reconstructed by the split-table kernel (batched API) */
    RS_STAT_REC_STRIPES_SYNDROME = 8, /* ... by the bit-sliced syndrome kernels                     */
    RS_STAT_ENCODE_BATCHES = 9,    /* rs_encode_batch GPU passes (one per staging group) */
    RS_STAT_MAILBOX_CALLS = 10,    /* rs_encode / rs_decode calls whose chunks went to a mailbox grid */
    RS_STAT_MAILBOX_RECOVERED = 11, /* ... of them with a chunk the grid left undone (launched by the caller) */
    RS_STAT_UPDATE_STRIPES = 12,   /* stripes patched by rs_update_stripes             */
    RS_STAT_UPDATE_COPY_COMMITS = 13, /* rs_update_stripes calls whose data commit ran as a separate copy pass */
    RS_STAT_READ_REGENERATED = 14, /* shards regenerated by rs_read_stripes            */
    RS_STAT_READ_COPIED = 15,      /* shards rs_read_stripes served by copy            */
    RS_STAT_CHECK_STRIPES = 16,    /* degraded stripes checked by the check kernel (rs_verify_degraded, rs_correct_degraded) */
    RS_STAT_SCRUB_REGENERATED = 17, /* shards regenerated by rs_correct_degraded       */
    RS_STAT_COMBINE_JOBS = 18,     /* jobs coded by rs_combine                         */
    RS_STAT_COMBINE_ROWS = 19,     /* output rows written by rs_combine                */
    RS_STAT_UPDATE_DEGRADED = 20,  /* stripes patched by the rs_update_degraded kernel */
    RS_STAT_UPDATE_ABSORBED = 21,  /* erased changed shards rs_update_degraded took into the parity only */
    RS_STAT_COLUMN_STRIPES = 22,   /* inconsistent stripes rs_correct_columns handed to the column kernel */
    RS_STAT_COLUMN_BYTES = 23,     /* bytes rs_correct_columns corrected                */
    RS_STAT_BATCH_LENS_PASSES = 24, /* GPU passes of rs_encode_batch_lens / rs_decode_batch_lens (one per staging group) */
    RS_STAT_COMBINE_LENS_LAUNCHES = 25, /* rs_combine_lens calls served by the per-job-length kernel (not by rs_combine's) */
    RS_STAT_REPAIR_CHECKED = 26,   /* stripes repaired and checked by the repair kernel (rs_reconstruct_checked*) */
    RS_STAT_SCRUB_LENS_LAUNCHES = 27, /* rs_verify_ptrs_lens / rs_reconstruct_checked_ptrs_lens calls served by the per-stripe-length kernels */
    RS_STAT_COLUMN_LENS_LAUNCHES = 28, /* column launches of rs_correct_columns_ptrs_lens served by the per-job-length twin (not by rs_correct_columns_ptrs') */
    RS_STAT_CRC_SECTORS = 29,      /* sectors checksummed by the rs_crc32c_* calls and rs_correct_crc32c */
    RS_STAT_CRC_REGENERATED = 30,  /* shards regenerated by rs_correct_crc32c          */
};
int64_t rs_stat(const rs_ctx *ctx, int which);

/* Diagnostics: the decode rows the engine uses for one erasure pattern
 * (erased = n flags).  rows receives m*k bytes: row t (t < *count) is the
 * combination of the k survivors (Rebuild's choice) that regenerates the
 * t-th erased shard in increasing id order; built on the GPU like every
 * batched pattern.  Synchronises the ctx's device. */
int rs_pattern_rows(rs_ctx *ctx, const uint8_t *erased, uint8_t *rows, int *count);
/* The shard ids behind the columns of those rows: ids[c] (k entries) is the
 * survivor that column c of rs_pattern_rows' rows multiplies for the same
 * flags -- slot i holds shard i if it is present, otherwise the
 * highest-numbered remaining parity (Rebuild's choice).  With it a caller
 * splits a decode row by holder for rs_combine without restating that rule.
 * RS_ENOT_ENOUGH for more than m erasures.  Host arithmetic only. */
int rs_pattern_survivors(const rs_ctx *ctx, const uint8_t *erased, int *ids);

/* Precompute (invert and upload) the decode patterns of every erasure set of
 * 1..max_erasures shards (max_erasures <= m), e.g. the 1,470 patterns of
 * RS(10,4) with <= 4 erasures, so later rs_reconstruct_stripes calls only
 * index them.  RS_EINVAL if that would exceed 2^20 patterns. */
int rs_prepare_patterns(rs_ctx *ctx, int max_erasures, void *stream);

/* ---- signature hashing: batched BLAKE2b -----------
 * The plugin signs and verifies blake2b(serializeMessage(id, message)):
 * defaultHashPolicy = blake2b.New() (main.go:38-41), keys.Sign at
 * main.go:219-223 on the send side, crypto.Verify at main.go:82-89 after
 * every decode; the framing is serializeMessage (main.go:276-302).  These
 * hash many messages per launch (RFC 7693 BLAKE2b, unkeyed, digest_len 1..64
 * bytes; noise's policy is recalled to use the 32-byte digest, which is not
 * BLAKE2b-512 truncated: the digest length is part of the parameter block).
 * BLAKE2b chains a message's 128-byte blocks sequentially, so one message
 * runs on 4 lanes; batches of hundreds of messages or more pay off.
 *
 * rs_blake2b_batch: host messages msgs[i] of lens[i] bytes (any alignment)
 * -> out[i * digest_len ...].  Staged through pinned memory like
 * rs_decode_batch; returns when out is written. */
int rs_blake2b_batch(rs_ctx *ctx, int count, const uint8_t *const *msgs, const size_t *lens,
                     int digest_len, uint8_t *out);
/* rs_blake2b_device: device-resident messages.  msg_ptrs[count] (device
 * addresses, any alignment) and lens[count] are device arrays; order
 * (device, may be NULL) lists the messages longest first; out is device
 * memory of count * digest_len bytes.  Enqueued on stream. */
int rs_blake2b_device(rs_ctx *ctx, int count, const uint64_t *msg_ptrs, const uint64_t *lens,
                      const uint32_t *order, int digest_len, uint8_t *out, void *stream);
/* rs_blake2b: the hash policy the plugin uses (hp.HashBytes, main.go:38-41,
 * :219-223, :82-89) with a host/GPU crossover.  A single message, or a batch
 * whose longest chain dominates, is hashed on the host CPU (C BLAKE2b, one
 * thread per message up to the CPUs this process may use); a batch with
 * many messages in flight goes to the GPU kernel (rs_blake2b_batch).  The
 * choice compares the two paths' estimated times; the
 * digests are identical either way.  RSMI_HASH=host / gpu forces a side.
 * *where (may be NULL) reports the side taken: 0 host, 1 GPU.
 * Replaces: hp.HashBytes(serializeMessage(...)) at main.go:219-223 (sign) and
 * main.go:82-89 (verify). */
int rs_blake2b(rs_ctx *ctx, int count, const uint8_t *const *msgs, const size_t *lens, int digest_len,
               uint8_t *out, int *where);
/* rs_blake2b_host: host-only BLAKE2b of host messages on `threads` threads
 * (<= 0: the CPUs this process may use).  Needs no context and no GPU. */
int rs_blake2b_host(int count, const uint8_t *const *msgs, const size_t *lens, int digest_len, uint8_t *out,
                    int threads);

/* ---- memory helpers ------------------------------------------------------
 * Engine-pinned host memory (hipHostMalloc, mapped for the device).  The
 * engine keeps a registry of these ranges: rs_decode_batch recognises
 * survivors that lie in them (and are 16-byte aligned) without querying the
 * runtime, and its reconstruct kernel reads them over PCIe in place -- no
 * staging memcpy, no per-shard DMA (zero-copy receive, SURVEY.md §8f rank 1;
 * the reference copies every ShardData at Unmarshal, shard.pb.go:468-503,
 * and DeepCopy's every share, main.go:255-258). */
void *rs_pinned_alloc(size_t bytes); /* NULL on failure */
void rs_pinned_free(void *p);
/* Receive arena: one pinned range carved into 256-byte aligned slots by a
 * bump pointer (rs_shard_unmarshal_arena places ShardData in it).  Reset
 * recycles every slot; not thread-safe (one arena per receiving thread).
 * rs_arena_put copies bytes into a fresh slot with streaming stores, as
 * rs_shard_unmarshal_arena does: the lines go to DRAM instead of staying
 * dirty in the CPU's caches, where each of the kernel's PCIe reads would
 * have to snoop them out. */
typedef struct rs_arena rs_arena;
rs_arena *rs_arena_new(size_t bytes);            /* NULL on failure */
void *rs_arena_alloc(rs_arena *a, size_t bytes); /* NULL when full */
void *rs_arena_put(rs_arena *a, const void *data, size_t bytes); /* the slot, NULL when full */
void rs_arena_reset(rs_arena *a);
size_t rs_arena_used(const rs_arena *a);
void rs_arena_free(rs_arena *a);
int rs_device_alloc(rs_ctx *ctx, size_t bytes, void **out);
int rs_device_free(rs_ctx *ctx, void *p);
int rs_stream_sync(rs_ctx *ctx, void *stream);

/* ---- device sets: one context over several GPUs ---------------------------
 * north_star: "stripes are independent, so they are partitioned across the 8
 * GPUs of one node with no collectives on the encode path"; SURVEY.md §8e and
 * §7.5 ("one host thread + stream per GPU").  The plugin process that loads
 * this library (through the Go shim's NewFECOnDevices) uses every GPU of the
 * node through one context:
 *
 * rs_new_devices builds a context over `count` HIP devices (devices[i];
 * repeats allowed -- two members on one GPU).  Member i is an ordinary
 * single-device context on devices[i] (rs_member; owned by the set, never
 * freed by the caller) with one host worker thread of its own.  Peer access
 * is enabled between every pair of distinct member devices that supports it.
 * Every entry point above accepts a device-set context:
 *  - rs_encode / rs_decode (one message) run on the member with the fewest
 *    calls in flight (concurrent Receive goroutines spread over the GPUs);
 *  - rs_encode_batch / rs_decode_batch split the messages into `count`
 *    contiguous ranges (rs_partition), each range on its member's thread, all
 *    members at once; per-message status and the return value as on one GPU;
 *  - the device-resident calls (rs_encode_stripes, rs_reconstruct_stripes,
 *    rs_verify_stripes, rs_correct_stripes, rs_update_stripes, rs_read_stripes,
 *    rs_verify_degraded, rs_correct_degraded, rs_correct_columns, rs_update_degraded, rs_reconstruct_ptrs,
 *    rs_verify_ptrs, rs_correct_columns_ptrs, rs_reconstruct_checked, rs_reconstruct_checked_ptrs,
 *    rs_verify_ptrs_lens, rs_reconstruct_checked_ptrs_lens, rs_correct_columns_ptrs_lens,
 *    rs_crc32c_stripes, rs_crc32c_check_stripes, rs_crc32c_ptrs, rs_crc32c_check_ptrs, rs_correct_crc32c,
 *    rs_fill_splitmix, rs_blake2b_device) run on a member on the device that holds their (first) device buffer, RS_EINVAL
 *    if no member is on it; rs_prepare_patterns (stream must be NULL) runs
 *    on every member; rs_blake2b* on the least-busy member;
 *  - rs_stat / rs_pattern_count / rs_pattern_evictions are summed over the
 *    members; rs_pattern_rows / rs_kernel_name / rs_device / rs_device_alloc
 *    are member 0's.
 * A single-device context is a set of one for the calls below. */
int rs_new_devices(int k, int n, const int *devices, int count, rs_ctx **out);
int rs_member_count(const rs_ctx *ctx);          /* 1 for a single-device context */
rs_ctx *rs_member(rs_ctx *ctx, int i);           /* NULL if i is out of range; owned by
                                                    the set (rs_free on it does nothing) */

/* Contiguous partition of `units` (stripes, messages) into `parts` ranges:
 * part p covers [*first, *first + *count) with first = units*p/parts, so the
 * ranges tile [0, units) in order and differ in size by at most one. */
int rs_partition(size_t units, int parts, int part, size_t *first, size_t *count);

/* Device-resident stripes already placed per member (stripe-local placement,
 * the headline): part i describes the stripes member i holds, in that
 * member's device memory, laid out as for rs_encode_stripes; stream is a
 * stream of member i's device or NULL.  All members' launches are issued
 * concurrently, one host thread per member; returns when every part is
 * queued (RS_OK, or the first failing status in member order). */
typedef struct rs_stripe_part {
    void *data;
    size_t data_stripe_stride;
    void *parity;
    size_t parity_stripe_stride;
    size_t stripes;
    void *stream;
} rs_stripe_part;
int rs_encode_stripes_parts(rs_ctx *ctx, const rs_stripe_part *parts, size_t shard_pitch, size_t shard_len);
/* erased: HOST flags [sum of parts' stripes][n], in part order (part i's
 * stripes follow part i-1's). */
int rs_reconstruct_stripes_parts(rs_ctx *ctx, const rs_stripe_part *parts, size_t shard_pitch, size_t shard_len,
                                 const uint8_t *erased);

/* Shard-distributed placement (the device analogue of the
 * plugin sending every shard to a different peer, main.go:207): shard i of
 * stripe s lives on ANY member's device, at the device address
 * shard_ptrs[s * n + i] (a HOST array; 16-byte aligned).  owner[s] (HOST) is
 * the member that reconstructs stripe s: its kernel reads Rebuild's survivors
 * where they lie -- over xGMI when they sit on another GPU (peer access, no
 * staging copy, no collective) -- and writes each erased shard at its address
 * (local or peer).  streams[i] (may be NULL, or hold NULLs) is member i's
 * stream; the survivors must be complete when those streams run.  Returns
 * when every member's launch is queued; RS_EDEVICE when the set spans devices
 * without peer access. */
int rs_reconstruct_spread(rs_ctx *ctx, const uint64_t *shard_ptrs, const int *owner, size_t shard_len,
                          size_t stripes, const uint8_t *erased, void *const *streams);

/* ---- bench / test utility (not on the codec path) ------------------------
 * Fill len bytes of device memory with the splitmix64 byte stream of seed
 * (byte i = byte i%8 of splitmix64(seed + (i/8 + 1) * golden)), the same
 * stream the CPU baseline generates. */
int rs_fill_splitmix(rs_ctx *ctx, void *dev, size_t len, uint64_t seed, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RSMI_H */

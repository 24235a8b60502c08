/*
 * sdgpu.h -- C ABI of libsdgpu.so: MI355X (gfx950) content identification for
 * Spacedrive's sd-core.
 *
 * This is the drop-in boundary for the hot path named in BASELINE.json: the
 * sampled-BLAKE3 cas_id, the full-file BLAKE3 integrity checksum and the
 * cas_id -> Object grouping step.  Every entry point below replaces a
 * reference function; the replaced interface is cited (file:line, paths
 * relative to the Spacedrive repository).  INTEGRATION.md shows the Rust FFI
 * binding (`extern "C"` block + wrappers keeping the reference signatures).
 *
 * Conventions
 *  - Plain C types only; no C++ or torch types cross this boundary.
 *  - Return value: 0 on success, a negative errno on failure (-EINVAL bad
 *    argument, -ENOMEM allocation, -ENODEV no usable GPU, -EIO HIP runtime
 *    error, or the -errno of a failed open/read/seek).  Per-item statuses use
 *    the same encoding, so a Rust caller maps them with
 *    io::Error::from_raw_os_error(-status) (FileIOError, core/src/util/error.rs:5-20).
 *  - "_device" entry points take device pointers and a hipStream_t passed as
 *    `void* stream` (NULL = the context's own stream, a blocking stream ordered
 *    with the null stream) and return without
 *    synchronising; all others take host pointers and return when done.
 *  - A context is used by one host thread at a time (the reference runs one
 *    job at a time, core/src/job/manager.rs:32); its device workspace is
 *    shared by all calls made through it.
 *  - Hex formatting stays with the caller: cas_id = lowercase hex of the 8
 *    returned bytes (cas.rs:61 `to_hex()[..16]`), checksum = lowercase hex of
 *    the 32 returned bytes (validation/hash.rs:21-23).  The path-based helpers
 *    additionally return the formatted strings.
 */
#ifndef SDGPU_H
#define SDGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDGPU_ABI_VERSION 6

/* cas.rs:10-15 */
#define SDGPU_CAS_SAMPLE_COUNT 4u
#define SDGPU_CAS_SAMPLE_SIZE 10240u
#define SDGPU_CAS_HEADER_OR_FOOTER_SIZE 8192u
#define SDGPU_CAS_MINIMUM_FILE_SIZE 102400u
/* Largest cas message: u64 size || whole 100 KiB file. */
#define SDGPU_CAS_MAX_MSG_LEN (8u + SDGPU_CAS_MINIMUM_FILE_SIZE)
/* Message of a sampled (> 100 KiB) file: 8 + 8192 + 4 * 10240 + 8192. */
#define SDGPU_CAS_SAMPLED_MSG_LEN 57352u
/* identifier_job_step batch size, file_identifier/mod.rs:36 */
#define SDGPU_IDENTIFIER_CHUNK_SIZE 100u

typedef struct sdgpu_ctx sdgpu_ctx;

int sdgpu_abi_version(void);
const char *sdgpu_strerror(int rc);

/* ---- context / memory ------------------------------------------------------ */
int sdgpu_device_count(int *count);
int sdgpu_open(int device, sdgpu_ctx **out);
/* Frees the context.  Destroy its indexes (sdgpu_index_destroy) and
 * communicators (sdgpu_comm_destroy) first: they point into it. */
int sdgpu_close(sdgpu_ctx *ctx);
/* Waits for all work issued through ctx (its stream and the last stream
 * passed to a _device call). */
int sdgpu_sync(sdgpu_ctx *ctx);
/* The context's hipStream_t. */
void *sdgpu_stream(sdgpu_ctx *ctx);
int sdgpu_alloc_pinned(sdgpu_ctx *ctx, size_t bytes, void **out);
int sdgpu_free_pinned(sdgpu_ctx *ctx, void *p);
int sdgpu_alloc_device(sdgpu_ctx *ctx, size_t bytes, void **out);
int sdgpu_free_device(sdgpu_ctx *ctx, void *p);
/* Asynchronous copy on `stream` (direction inferred by the runtime). */
int sdgpu_memcpy_async(sdgpu_ctx *ctx, void *dst, const void *src, size_t bytes, void *stream);

/* ---- K1: sampled cas_id ------------------------------------------------------
 * Replaces the hashing of generate_cas_id (core/src/object/cas.rs:23-62) for a
 * whole batch of files (identifier_job_step, file_identifier/mod.rs:107-134).
 * Message i is msg_arena[msg_off[i] .. msg_off[i] + msg_len[i]) and must be
 * the exact byte sequence the reference feeds its Hasher:
 *   u64 size little-endian || file bytes          (size <= 100 KiB, cas.rs:27-29)
 *   u64 size LE || file[0,8192) || 4 x file[8192 + k*((size-16384)/4), +10240)
 *     || file[len-8192, len)                       (size > 100 KiB, cas.rs:30-58)
 * msg_off[i] % 16 == 0 and msg_len[i] <= SDGPU_CAS_MAX_MSG_LEN, else
 * status[i] = -EINVAL and out8[i] is zeroed.  out8[i] = BLAKE3(M_i)[0..8).
 * status may be NULL. */
int sdgpu_cas_batch(sdgpu_ctx *ctx, const uint8_t *msg_arena, const uint64_t *msg_off,
                    const uint32_t *msg_len, uint32_t n, uint8_t (*out8)[8], int32_t *status);
/* Device-resident variant.  arena_bytes bounds the arena and sizes the K1
 * workspace (arena_bytes / 1024 + n chaining-value slots, enough for disjoint
 * messages inside the arena).  A message ending past arena_bytes gets
 * status -EINVAL.  Messages may overlap (e.g. duplicates sharing one copy) as
 * long as their 4-chunk units plus n fit that bound; otherwise EVERY message
 * gets -ENOBUFS and nothing is hashed (no write past the workspace). */
int sdgpu_cas_batch_device(sdgpu_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes,
                           const uint64_t *d_off, const uint32_t *d_len, uint32_t n,
                           uint8_t *d_out8, int32_t *d_status, void *stream);
/* (ABI 6, additive) sdgpu_cas_batch_device plus the integrity_checksum of the
 * files read whole: d_out8 and d_status are exactly what sdgpu_cas_batch_device
 * gives for the same arguments.  d_whole is device u8[n]: message i with
 * d_whole[i] != 0 is u64 size LE || a whole file (cas.rs:27-29), and for every
 * such message with status 0 and len >= 8, d_out32[i] (device [n][32], 4-B
 * aligned) = BLAKE3(arena[off + 8 .. off + len)) -- file_checksum of those
 * bytes (hash.rs:10-24) -- and d_has_checksum[i] (device u8[n]) = 1.  Every
 * other message gets 32 zero bytes and d_has_checksum 0; under -ENOBUFS that
 * is every message.  The digests come from a second K1 pass over the message
 * bodies on the same stream; no byte at or beyond off + len is read.  NULL
 * d_whole, d_out32 or d_has_checksum with n > 0 is -EINVAL. */
int sdgpu_cas_checksum_batch_device(sdgpu_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes,
                                    const uint64_t *d_off, const uint32_t *d_len,
                                    const uint8_t *d_whole, uint32_t n, uint8_t *d_out8,
                                    uint8_t *d_out32, uint8_t *d_has_checksum, int32_t *d_status,
                                    void *stream);

/* Pinned-host staged variant (the identifier's "pinned async staging", BASELINE
 * config 5): the messages live in caller-owned PINNED host memory (e.g. where
 * the pread of the cas windows landed, sdgpu_alloc_pinned), in file order
 * (h_off ascending, 16-B aligned).  The library streams the arena through a
 * ring of device slabs -- H2D on its own copy stream overlapped with K1 on
 * `stream` -- and leaves the cas bytes in device memory (d_out8 [n][8],
 * d_status [n] or NULL) for the grouping step.  Asynchronous: h_arena must
 * stay untouched until sdgpu_sync; h_off/h_len are consumed before return. */
int sdgpu_cas_stage_pinned(sdgpu_ctx *ctx, const uint8_t *h_arena, const uint64_t *h_off,
                           const uint32_t *h_len, uint32_t n, uint8_t *d_out8, int32_t *d_status,
                           void *stream);

/* Path-based drop-in for generate_cas_id(path, size) (cas.rs:23): same reads
 * as the reference (open, header, 4 samples by seek, footer from the actual
 * end), hash on the GPU, out_hex = 16 lowercase hex chars + NUL. */
int sdgpu_generate_cas_id(sdgpu_ctx *ctx, const char *path, uint64_t size, char out_hex[17]);

/* Batched file identifier staging (file_identifier/mod.rs:107-134 join_all of
 * FileMetadata::new -> generate_cas_id): reads the cas windows of n files with
 * pread into pinned buffers, pipelines H2D copies with K1 in slabs.  size[i] is
 * the fs::metadata length (mod.rs:65,80-81); size 0 yields status 0 and
 * has_key[i] = 0 (cas_id None, mod.rs:80-88); I/O errors yield status -errno
 * and has_key 0 (row dropped, mod.rs:113,127).  has_key may be NULL.
 * size may be NULL (ABI 6): every path is stat-ed by the read pool first --
 * the reference's fresh fs::metadata(path).len() at identification time, not
 * a size stored with the row; a failed stat is status -errno, a directory
 * -EISDIR (the reference asserts the path is not one, mod.rs:69-72). */
int sdgpu_identify_files(sdgpu_ctx *ctx, const char *const *paths, const uint64_t *size,
                         uint32_t n, uint8_t (*out8)[8], uint8_t *has_key, int32_t *status);
/* (ABI 6, additive) sdgpu_identify_files that also returns the
 * integrity_checksum of every file it read whole, from the same read: out8,
 * has_key and status are exactly what sdgpu_identify_files gives.
 * has_checksum[i] = 1 iff status[i] is 0 and the size used (the one passed, or
 * the one stat-ed when size is NULL) is in (0, 100 KiB]; out32[i] is then
 * BLAKE3 of the bytes the call read -- the bytes that went into the cas_id,
 * what file_checksum(path) (hash.rs:10-24) would have returned at that moment,
 * also for a file that grew since its size was taken.  Every other row (size
 * 0: not opened; sampled files; failed rows) gets has_checksum 0 and 32 zero
 * bytes, and is left to the object validator (sdgpu_checksum_files).  out32
 * and has_checksum must not be NULL when n > 0. */
int sdgpu_identify_checksum_files(sdgpu_ctx *ctx, const char *const *paths, const uint64_t *size,
                                  uint32_t n, uint8_t (*out8)[8], uint8_t *has_key,
                                  uint8_t (*out32)[32], uint8_t *has_checksum, int32_t *status);

/* ---- Object kind (ABI 6, additive) -------------------------------------------
 * The third output of FileMetadata::new (file_identifier/mod.rs:75-78):
 * Extension::resolve_conflicting(&path, false) of sd-file-ext, as ObjectKind
 * values (crates/file-ext/src/kind.rs).  One table (215 extension variants,
 * 127 signature alternatives) and one matcher serve the host calls and the
 * kernel.  flags: 0 = the identifier's mode (always_check_magic_bytes =
 * false: a name of one category gives that category with no byte looked at;
 * `ts` / `mts` are Video when the Video signature matches, else Code), or
 * SDGPU_KIND_VERIFY_MAGIC = the function's second parameter set (names of
 * Image, Audio, Video, Archive, Executable, Font, Encrypted, Mesh, Database
 * keep their category only when their signature matches, else kind 0).  Any
 * other flag bit is -EINVAL.  A path without an Extension has kind 0 (Unknown). */
#define SDGPU_KIND_VERIFY_MAGIC 1u
/* (ABI 6, additive) ext_id_out[i] = extension id of paths[i] (magic.rs:180-186:
 * Path::extension, to_str, to_lowercase, Extension::from_str): 0 = no
 * Extension, else 1..215, stable.  Host only, no context. */
int sdgpu_kind_ext_ids(const char *const *paths, uint32_t n, uint16_t *ext_id_out);
/* (ABI 6, additive) Enumerates the table (extensions.rs:11-362): out = the
 * lower-case name of ext_id (NUL-padded), kinds[0] its ObjectKind, kinds[1] 0
 * except for the entries `ts` / `mts` resolve to, where it is Code (kinds[0]
 * Video); -ENOENT for 0 and past the end.  A path resolves to the first entry
 * of its name. */
int sdgpu_kind_ext_name(uint32_t ext_id, char out[16], int32_t kinds[2]);
/* (ABI 6, additive) resolve_conflicting(path, flags) as the reference does it
 * (magic.rs:176-236): the file is opened when its name has an Extension, and
 * read (its first bytes only) when the decision needs them.  *kind = 0 and
 * return 0 when the open fails (magic.rs:188-190).  Host only. */
int sdgpu_kind_of_file(const char *path, uint32_t flags, int32_t *kind);
/* (ABI 6, additive) Kinds of n device-resident cas messages (magic.rs:160-236):
 * d_ext is device u16[n] (sdgpu_kind_ext_ids), d_kind device u8[n].  The file
 * bytes of message i are arena[off + 8 .. off + len); a message shorter than
 * 8 bytes has none.  Validity as in sdgpu_cas_batch_device (offset 16-B
 * aligned, len <= SDGPU_CAS_MAX_MSG_LEN, inside arena_bytes): an invalid
 * message gets kind 0.  Reads at most the first 48 bytes of a message, never
 * a byte at or beyond off + len; the arena is not written.  Asynchronous on
 * `stream`. */
int sdgpu_kind_batch_device(sdgpu_ctx *ctx, const uint8_t *d_arena, uint64_t arena_bytes,
                            const uint64_t *d_off, const uint32_t *d_len, const uint16_t *d_ext,
                            uint32_t n, uint32_t flags, uint8_t *d_kind, void *stream);
/* (ABI 6, additive) sdgpu_identify_files that also returns each file's kind
 * (mod.rs:59-97 whole), from the bytes the call read for the cas_id: out8,
 * has_key and status are exactly what sdgpu_identify_files gives; out32 and
 * has_checksum are either both NULL (no body pass) or exactly what
 * sdgpu_identify_checksum_files gives.  kind[i] (int32, required) is defined
 * for rows with status 0 -- empty files included: they are opened and closed
 * when their name has an Extension, a failure giving kind 0 with status still
 * 0 -- and 0 for failed rows.  The bytes tested are the bytes that went into
 * the cas_id, also for a file that changed since its size was taken. */
int sdgpu_identify_kind_files(sdgpu_ctx *ctx, const char *const *paths, const uint64_t *size,
                              uint32_t n, uint32_t flags, uint8_t (*out8)[8], uint8_t *has_key,
                              uint8_t (*out32)[32], uint8_t *has_checksum, int32_t *kind,
                              int32_t *status);

/* ---- K2/K3: full-file checksum -------------------------------------------------
 * Replaces file_checksum (core/src/object/validation/hash.rs:10-24). */
/* BLAKE3 of a host buffer. */
int sdgpu_checksum(sdgpu_ctx *ctx, const void *bytes, uint64_t len, uint8_t out32[32]);
/* BLAKE3 of n device-resident files (pointers 16-B aligned); d_files and lens
 * are HOST arrays of device addresses / byte lengths, d_out32 is device [n][32]. */
int sdgpu_checksum_batch_device(sdgpu_ctx *ctx, const uint8_t *const *d_files,
                                const uint64_t *lens, uint32_t n, uint8_t *d_out32, void *stream);
/* Chaining value of one aligned subtree slice (for streaming hosts): len bytes
 * starting at chunk counter chunk_offset; chunk_offset must be a multiple of
 * the slice's chunk count (ceil(len / 1024)) rounded up to a power of two, else
 * -EINVAL; a slice of at most one chunk may sit at any counter.  root=1 gives
 * the digest of a whole message (chunk_offset 0). */
int sdgpu_subtree_device(sdgpu_ctx *ctx, const uint8_t *d_bytes, uint64_t len,
                         uint64_t chunk_offset, int root, uint8_t *d_out32, void *stream);
/* Digest of a message from the chaining values of its consecutive aligned
 * subtree slices (sdgpu_subtree_device with root=0): d_cvs is device [n][32]
 * (16-B aligned), n >= 2, every slice of the same power-of-two chunk count
 * except a shorter last one.  One large file split over several GPUs: each
 * GPU computes its slices' CVs, one GPU combines them. */
int sdgpu_combine_subtrees_device(sdgpu_ctx *ctx, const uint8_t *d_cvs, uint64_t n,
                                  uint8_t *d_out32, void *stream);
/* Latency service for the single-file callers (watcher/utils.rs:236,411,467,
 * non_indexed.rs:161): with enable != 0, sdgpu_generate_cas_id and
 * sdgpu_file_checksum hash messages of at most 112 KiB (every cas message;
 * files up to 112 KiB for the checksum) on a workgroup that stays resident
 * on the device and polls a mailbox in pinned memory -- no launch, copy
 * command or stream synchronisation per call.  The workgroup occupies part
 * of one CU until 20 ms after the last such call (then it ends itself; the
 * next call restarts it) and is stopped before any other call of the context
 * launches work.
 * Crossover for the watcher / non-indexed callers (MI355X, measured,
 * profiles/r3/check_r3R_bench.json): the workgroup hashes in quads of lanes
 * (one compression spread over 4 lanes); generate_cas_id through the service
 * 23 / 25 / 28 / 35 us at 4 / 16 / 32 / 64 KiB and 32 us for a sampled file
 * (57 352-B message), against 7.7 / 22 / 40 / 78 / 69 us on one CPU thread
 * of the AVX2 port.  So: hash on the CPU below ~20 KiB of message, on the
 * GPU above (every file > 100 KiB for generate_cas_id; files > 20 KiB for
 * file_checksum, where 1 MiB takes 78 us vs 1.1 ms). */
int sdgpu_latency_service(sdgpu_ctx *ctx, int enable);
/* Path-based drop-in for file_checksum(path): streams the file in 64 MiB
 * power-of-two slices through double-buffered pinned memory; out_hex = 64
 * lowercase hex chars + NUL. */
int sdgpu_file_checksum(sdgpu_ctx *ctx, const char *path, char out_hex[65]);

/* Batched object validator: file_checksum of n files (validator_job.rs:126-169
 * checksums one file per job step).  Files up to 16 MiB are read whole by a
 * thread pool into pinned slabs and each slab is hashed by one tree launch;
 * larger files are streamed like sdgpu_file_checksum.  out32[i] = BLAKE3 of
 * file i (lowercase hex of it = the reference's integrity_checksum);
 * status[i] = 0 or -errno (out32 zeroed), status may be NULL. */
int sdgpu_checksum_files(sdgpu_ctx *ctx, const char *const *paths, uint32_t n,
                         uint8_t (*out32)[32], int32_t *status);

/* ---- K4-K6: cas_id -> Object grouping ------------------------------------------
 * Replaces the Object link/create decisions of identifier_job_step
 * (file_identifier/mod.rs:167-333) over the orphan rows in ascending id order
 * processed in chunks of chunk_rows (=100, mod.rs:36; file_identifier_job.rs:286-309).
 * Rows are identified by their rank r (position in id order, < 2^31).  Output
 * rep[r]: the rank of the row whose Object row r is linked to:
 *   - has_key[r] == 0 (empty file, cas_id None): rep[r] = r;
 *   - r in the chunk holding the lowest-rank row f of its key: rep[r] = r
 *     (a new Object per row, mod.rs:233-297);
 *   - otherwise rep[r] = f (linked to an existing Object, mod.rs:189-225).
 * key = the 8 cas bytes read as a little-endian u64 (equality is all the
 * grouping uses, mod.rs:136-141,196-203).
 * The calls below group the rows they are given.  Objects that exist BEFORE
 * the rows (earlier batches of the run, earlier runs, other locations: the
 * library-wide find_many of mod.rs:168-185) come from an Object index, see
 * sdgpu_index_* and sdgpu_group_rows_indexed_device. */
int sdgpu_dedup(sdgpu_ctx *ctx, const uint64_t *key, const uint8_t *has_key, uint32_t n,
                uint32_t chunk_rows, uint32_t *rep);
/* Device-resident, one GPU: rows given as (key, rank) pairs (rows without a
 * key are simply not passed); writes rep for each pair at the same index.
 * skip_bits: accepted for ABI 1 compatibility and ignored (bucket digits come
 * from a hash of the key since ABI 2, so shards need no skipped bits). */
int sdgpu_group_pairs_device(sdgpu_ctx *ctx, const uint64_t *d_key, const uint32_t *d_rank,
                             uint64_t n, uint32_t chunk_rows, uint32_t skip_bits, uint32_t *d_rep,
                             void *stream);
/* Device-resident, one GPU, whole rows: rep[i] for every row i; rows with
 * d_has_key[i] == 0 get rep[i] = rank[i].  d_has_key NULL = every row keyed;
 * d_rank NULL = rank i (rows already in id order; the partition then moves
 * 12-byte bucket records instead of 16-byte ones, ~10 % faster).  skip_bits
 * ignored. */
int sdgpu_group_rows_device(sdgpu_ctx *ctx, const uint64_t *d_key, const uint8_t *d_has_key,
                            const uint32_t *d_rank, uint64_t n, uint32_t chunk_rows,
                            uint32_t skip_bits, uint32_t *d_rep, void *stream);

/* ---- Object index: Objects that exist before a batch ------------------------
 * Replaces the library-wide lookup of identifier_job_step
 * (file_identifier/mod.rs:168-185: Objects owning a file_path whose cas_id is
 * in the step's set) and the link of matching rows to them (:189-225, :233-241).
 * A device hash table key -> value lives with one context.  Values are either
 * a row rank (the Object created by that row in an earlier batch of the same
 * run) or SDGPU_REP_EXISTING | handle for an Object registered by the caller
 * (handle < 2^31, e.g. the Object's database id).  A key keeps the canonical
 * "first" Object: a registered (pre-existing) Object before any
 * Object created during the run, whatever the order of the calls (find_many,
 * mod.rs:168-185, returns Objects already in the database); the lowest handle
 * among registered ones, the lowest rank among created ones.  Row ranks must
 * be < 2^31 (SDGPU_REP_EXISTING is the top bit).
 * Grouping batches in id order through one index yields exactly the grouping
 * of the whole run (tests/test_gpu_index.py). */
#define SDGPU_REP_EXISTING 0x80000000u
typedef struct sdgpu_index sdgpu_index;
int sdgpu_index_create(sdgpu_ctx *ctx, uint64_t capacity_hint, sdgpu_index **out);
int sdgpu_index_destroy(sdgpu_index *idx);
int sdgpu_index_clear(sdgpu_index *idx, void *stream);
/* Distinct keys stored: live keys, removed ones not counted (synchronises). */
int sdgpu_index_count(sdgpu_index *idx, uint64_t *count);
/* Register pre-existing Objects: d_key[i] -> SDGPU_REP_EXISTING | d_handle[i].
 * Only keys whose shard belongs to `rank` of `world` are kept (world = 1: all),
 * so every GPU of a sharded grouping can be given the same list.  May
 * synchronise `stream` when the table grows. */
int sdgpu_index_add_objects_device(sdgpu_index *idx, const uint64_t *d_key,
                                   const uint32_t *d_handle, uint64_t n, uint32_t world,
                                   uint32_t rank, void *stream);

/* ---- a library-lifetime index (ABI 6, additive) -------------------------------
 * An index that outlives one identifier job has to follow what the reference
 * does to Objects behind the identifier's back: the orphan remover deletes
 * Objects by id (core/src/object/orphan_remover.rs:57-90), the watcher's
 * delete / update paths delete an Object left without file_paths
 * (location/manager/watcher/utils.rs:746-765) and its create path asks "does
 * an Object own this cas_id" for one file (utils.rs:240-275).  The calls
 * below answer and maintain that; a grouping through the index afterwards
 * treats a removed key as one the library-wide find_many no longer returns
 * (its next row creates an Object again).
 * A removed entry keeps its slot until the table is next rebuilt (growth
 * drops removed slots and sizes the new table from the live keys, so
 * capacity stays bounded under churn); inserting the key again revives it.
 * LIMIT: the index keeps ONE Object per key, the lowest registered handle.
 * When that Object is removed while another Object still owns the same
 * cas_id, the index forgets the key: the caller re-registers the survivor
 * with sdgpu_index_add_objects_device (it has it: the reference's own query
 * for such Objects is mod.rs:168-175).
 * Sharded index (add_objects with world > 1): every rank's share may be given
 * the same key / handle lists; keys of other shards are simply absent. */
/* (ABI 6, additive) sdgpu_index_lookup's value for a key the index does not hold. */
#define SDGPU_INDEX_MISS 0xFFFFFFFFu
/* (ABI 6, additive) d_value[i] = the stored value of d_key[i], exactly as a
 * grouping's rep would show it (a row rank, or SDGPU_REP_EXISTING | handle),
 * SDGPU_INDEX_MISS when the key is absent or removed.  A pure read: does not
 * grow the table, does not synchronise.  A share of a sharded index misses
 * the keys of the other shards: the caller takes the non-miss answer across
 * the shares. */
int sdgpu_index_lookup_device(sdgpu_index *idx, const uint64_t *d_key, uint64_t n,
                              uint32_t *d_value, void *stream);
/* (ABI 6, additive) The same on host arrays (the watcher's single-file case):
 * copy in, one launch, copy out; returns when done. */
int sdgpu_index_lookup(sdgpu_index *idx, const uint64_t *key, uint64_t n, uint32_t *value);
/* (ABI 6, additive) Removes d_key[0..n).  d_value (may be NULL): key i is
 * removed only while its stored value equals d_value[i] (an Object that took
 * the key over since the caller looked is left alone).  d_removed (device
 * uint32_t, may be NULL) receives the number of keys actually removed: a key
 * listed several times counts once, an absent key not at all. */
int sdgpu_index_remove_device(sdgpu_index *idx, const uint64_t *d_key, const uint32_t *d_value,
                              uint64_t n, uint32_t *d_removed, void *stream);
/* (ABI 6, additive) Removes every entry whose value is SDGPU_REP_EXISTING | h
 * for an h in d_handle[0..n) -- the orphan remover's shape: it knows Object
 * ids, not cas_ids.  The ids sdgpu_orphan_objects_device writes are usable
 * directly as d_handle (negative ids and ids above max_handle match nothing);
 * max_handle < 2^31 sizes the mark map (max_handle + 1 bytes of the context's
 * workspace, as sdgpu_orphan_objects_device).  One pass over the slots;
 * entries holding row ranks are never touched.  d_removed as above. */
int sdgpu_index_remove_objects_device(sdgpu_index *idx, const int32_t *d_handle, uint64_t n,
                                      uint32_t max_handle, uint32_t *d_removed, void *stream);
/* (ABI 6, additive) The live entries as dense (key, value) arrays of at most
 * cap pairs, in no particular order (compare as a set), the key ~0 included;
 * values as sdgpu_index_lookup_device shows them.  d_count[0] (device) = the
 * number of live entries: when it exceeds cap nothing was written past cap
 * and the caller retries with larger arrays.  To load a saved index:
 * sdgpu_index_add_objects_device for the SDGPU_REP_EXISTING entries (rank
 * entries belong to the run that made them). */
int sdgpu_index_export_device(sdgpu_index *idx, uint64_t *d_key, uint32_t *d_value, uint64_t cap,
                              uint32_t *d_count, void *stream);
/* (ABI 6, additive) out = {live keys, slots in use including removed ones,
 * capacity in slots} (synchronises, like sdgpu_index_count). */
int sdgpu_index_stats(sdgpu_index *idx, uint64_t out[3]);

/* sdgpu_group_rows_device against the index: a keyed row whose key is in the
 * index gets rep = the index value if it is an existing Object, else (a rank
 * f of an earlier batch) rep = r when r and f share a chunk and f otherwise;
 * the other rows are grouped among themselves; afterwards every row that
 * created an Object (rep == rank) is inserted with its rank.  May synchronise
 * `stream` when the table grows. */
int sdgpu_group_rows_indexed_device(sdgpu_ctx *ctx, sdgpu_index *idx, const uint64_t *d_key,
                                    const uint8_t *d_has_key, const uint32_t *d_rank, uint64_t n,
                                    uint32_t chunk_rows, uint32_t *d_rep, void *stream);
/* Host arrays, one batch of n rows with ranks first_rank + i (an identifier
 * job step over a whole batch); idx may be NULL (group the batch alone). */
int sdgpu_dedup_batch(sdgpu_ctx *ctx, sdgpu_index *idx, const uint64_t *key,
                      const uint8_t *has_key, uint32_t first_rank, uint32_t n,
                      uint32_t chunk_rows, uint32_t *rep);

/* ---- multi-GPU grouping: hash-sharded over a node, RCCL all-to-all over xGMI --
 * Every key has one owner GPU (shard = top 8 bits of mix64(key), rank d owns
 * shards s with s * world / 256 == d); each GPU sends its keyed rows to their
 * owners as packed 12-byte {key, rank} records, the owners group their rows
 * (and probe their share of the Object index), and the reps return (4 B per
 * row).  Two exchanges (sdgpu_comm_set_exchange): COUNTED -- a count
 * all-to-all sizes the messages, one host synchronisation per call; PADDED
 * (ABI 5, the default once a communicator has run one call) -- every
 * (source, owner) message has a fixed capacity agreed by all ranks, its
 * real count travels in its first slot and is read on the device, and the
 * call enqueues everything without waiting for the host.
 * Transports: SDGPU_TRANSPORT_RCCL (grouped ncclSend/ncclRecv; one rank per
 * GPU), SDGPU_TRANSPORT_PEER (device-to-device copies between contexts of one
 * process; also contexts sharing a GPU), AUTO = RCCL unless devices repeat,
 * SDGPU_TRANSPORT_HOST (ABI 6, sdgpu_comm_init_host: one process per rank on
 * one host, ranks may share a GPU). */
#define SDGPU_COMM_ID_BYTES 128
#define SDGPU_TRANSPORT_AUTO 0
#define SDGPU_TRANSPORT_RCCL 1
#define SDGPU_TRANSPORT_PEER 2
#define SDGPU_TRANSPORT_HOST 3
typedef struct sdgpu_comm sdgpu_comm;
/* Failure model (ABI 3).  RCCL communicators are created non-blocking; every
 * wait on a peer (joining, the count exchange's one synchronisation,
 * sdgpu_comm_wait) is bounded by the communicator's timeout.  When it passes,
 * or a local step of the exchange fails, the communicator is aborted (its
 * queued kernels exit) and the call returns -ETIMEDOUT (or the local error);
 * the peers then time out too, so a missing or failed rank ends the job with
 * an error on every rank instead of a hang.  An aborted communicator returns
 * -ECONNABORTED from every later exchange; destroy it. */
int sdgpu_comm_unique_id(uint8_t id[SDGPU_COMM_ID_BYTES]);
/* One process per GPU: rank 0 creates the id, every rank receives it out of
 * band and joins; returns when all nranks have joined, or -ETIMEDOUT after
 * timeout_ms (> 0).  The timeout also bounds the communicator's exchanges. */
int sdgpu_comm_init_rank_timeout(sdgpu_ctx *ctx, int nranks, int rank,
                                 const uint8_t id[SDGPU_COMM_ID_BYTES], int timeout_ms,
                                 sdgpu_comm **out);
/* The same with the timeout from env SDGPU_COMM_TIMEOUT_MS (default 300 s). */
int sdgpu_comm_init_rank(sdgpu_ctx *ctx, int nranks, int rank,
                         const uint8_t id[SDGPU_COMM_ID_BYTES], sdgpu_comm **out);
/* One process per rank on one host, through a shared file mapping (ABI 6):
 * the same messages, in the same order, as the RCCL transport, staged
 * through host memory -- each rank's outbox of msg_bytes holds its messages
 * of one all-to-all round; a round waits for the rank's stream, posts the
 * outbox, waits (bounded by timeout_ms) for every peer's, copies its
 * inbound messages and waits until every peer has copied its own.  The
 * exchange calls (sdgpu_group_sharded_device, sdgpu_group_link_sharded_
 * device) run exactly the per-process state machine they run under RCCL
 * (a padded call left pending and resolved at the next call / wait / destroy,
 * the overflow re-run, the deferred -ENOSPC, the bounded failure), so ranks
 * that share a GPU -- which RCCL refuses -- can exercise it.  Host-
 * synchronous: a test and fallback transport, not a fast one.  path names a
 * file every rank opens (created by the first; it must not hold an earlier
 * communicator's state: -EEXIST); rank 0 unlinks it on destroy.  A round
 * whose messages exceed msg_bytes fails with -EMSGSIZE.  -ETIMEDOUT when not
 * every rank joins within timeout_ms (> 0), -EPROTO when the ranks disagree
 * on nranks or msg_bytes. */
int sdgpu_comm_init_host(sdgpu_ctx *ctx, int nranks, int rank, const char *path,
                         uint64_t msg_bytes, int timeout_ms, sdgpu_comm **out);
/* One process driving ngpu contexts: out[r] is rank r's communicator. */
int sdgpu_comm_init_all(sdgpu_ctx *const *ctx, int ngpu, int transport, sdgpu_comm **out);
int sdgpu_comm_destroy(sdgpu_comm *comm);
int sdgpu_comm_info(sdgpu_comm *comm, int *nranks, int *rank, int *transport);
int sdgpu_comm_set_timeout(sdgpu_comm *comm, int timeout_ms);
/* Waits, bounded by the timeout, until `stream` (NULL: the stream of the
 * communicator's last exchange) has drained -- i.e. the reps of the last
 * sdgpu_group_sharded_device are written -- and resolves a padded exchange
 * (below): if any message of it overflowed, the call is re-run through the
 * counted exchange before this returns.  Returns that call's result (e.g.
 * -ENOSPC of a write set that did not fit).  -ETIMEDOUT (communicator
 * aborted) if a peer never completes its side. */
int sdgpu_comm_wait(sdgpu_comm *comm, void *stream);
/* Exchange of the one-process-per-GPU calls (sdgpu_group_sharded_device,
 * sdgpu_group_link_sharded_device; ABI 5):
 *   COUNTED: counts first, then the records; one host synchronisation per
 *     call, the results final when the stream reaches them.
 *   PADDED: no host synchronisation.  The message from each source to each
 *     owner holds C = min(B, B / nranks + B / (128 nranks) + 4096) records
 *     (a little over its expected share; B = the largest n of the ranks'
 *     previous call, which every rank learns from the headers, or rows_hint)
 *     plus a header slot; the owners drop the padding on the device.  A
 *     message that needed more than C records (a cas_id held by many rows,
 *     a rank with more rows than B) sets an overflow bit every rank sees.
 *     The call is RESOLVED at the next exchange call on the communicator,
 *     sdgpu_comm_wait or destroy: overflowed calls are then re-run through
 *     the counted exchange on the same stream, on every rank alike.  Until
 *     it is resolved, the call's inputs must not change and its outputs are
 *     not final (read them after sdgpu_comm_wait).  The rep form with an
 *     explicit SDGPU_RETURN_COMPACT stays counted.
 *   AUTO (default): PADDED once B is known (after the first call), else
 *     COUNTED.
 * Every rank of a communicator must set the same mode (and rows_hint, which
 * sets B when > 0).  The _all entry points (one process, all ranks) resolve
 * a padded call before they return -- also with ngpu = 1, whose communicator
 * is a one-rank per-process one.
 * Agreement (ABI 6): a communicator's first call and its first call after
 * sdgpu_comm_set_exchange / sdgpu_comm_set_return (which every rank must
 * call alike, between the same two exchange calls) check that every rank
 * chose the same layout -- a counted call through the code in its count
 * messages (form, return mode, exchange mode), a padded call through one
 * 24-byte agreement message per peer {slots per message, B, code} of the
 * same shape, before any record moves -- and fail with -EPROTO (communicator
 * aborted) when they differ, instead of posting messages of different sizes.
 * -ENOSPC of a padded write set that is resolved by a later call is returned
 * by the next sdgpu_comm_wait (the earliest unreported one; stats.nospc_call
 * names the call); a hard error found by the same wait takes precedence. */
#define SDGPU_EXCHANGE_AUTO 0
#define SDGPU_EXCHANGE_COUNTED 1
#define SDGPU_EXCHANGE_PADDED 2
int sdgpu_comm_set_exchange(sdgpu_comm *comm, int mode, uint64_t rows_hint);
/* Cumulative exchange volume of this rank (bytes = 12-B records + 4-B reps). */
typedef struct sdgpu_comm_stats_t {
  uint64_t calls;
  uint64_t rows_sent, rows_received;      /* keyed rows to / from every rank incl. self */
  uint64_t bytes_sent, bytes_received;    /* payload incl. the self share: 12-B records,
                                             plus the reps this rank returned as an owner
                                             (sent) / got back as a source (received);
                                             padded calls: the whole fixed-size messages */
  uint64_t bytes_remote;                  /* payload that crossed to / from other ranks */
  double count_wait_ms;                   /* host ms until the counts were known (0 for
                                             padded calls) */
  double host_ms;                         /* host ms inside the exchange calls */
  uint64_t rows_returned;                 /* (ABI 4) received rows whose rep went back */
  uint64_t padded_calls;                  /* (ABI 5) calls through the padded exchange */
  uint64_t overflow_reruns;               /* (ABI 5) padded calls re-run counted */
  double resolve_wait_ms;                 /* (ABI 5) host ms waiting to resolve them */
  uint64_t agreements;                    /* (ABI 6) layout agreement rounds (below) */
  uint64_t nospc_call;                    /* (ABI 6) `calls` number of the last call that
                                             failed with -ENOSPC (0: none) */
} sdgpu_comm_stats_t;
/* Return leg of the exchange (ABI 4).  COMPACT: an owner sends back only the
 * received rows whose rep is not their own rank, as 8-B {index, rep} pairs
 * after a second count exchange (a second host synchronisation); ~1.6 B per
 * row instead of 4 at config 4's 20 % duplicates.  FULL: every received row's
 * 4-B rep, one synchronisation per call.  AUTO (the default): COMPACT when the
 * largest rank's rows / nranks >= 4 Mi (the bytes it saves per link outweigh
 * the second synchronisation), else FULL -- decided per call from every
 * rank's n, which travels with the counts, so all ranks agree.  All ranks of
 * a communicator must set the same mode. */
#define SDGPU_RETURN_FULL 0
#define SDGPU_RETURN_COMPACT 1
#define SDGPU_RETURN_AUTO 2
int sdgpu_comm_set_return(sdgpu_comm *comm, int mode);
int sdgpu_comm_stats(sdgpu_comm *comm, sdgpu_comm_stats_t *out);
/* Collective, one process per GPU (RCCL): every rank calls it with its own
 * rows (global ranks in d_rank, required, each < 2^31); rep for each of its
 * rows.  idx (may be NULL) is this rank's share of the Object index. */
int sdgpu_group_sharded_device(sdgpu_ctx *ctx, sdgpu_comm *comm, sdgpu_index *idx,
                               const uint64_t *d_key, const uint8_t *d_has_key,
                               const uint32_t *d_rank, uint64_t n, uint32_t chunk_rows,
                               uint32_t *d_rep, void *stream);
/* The same from one process for all ngpu ranks at once (arrays indexed by
 * rank; idx, d_has_key and streams may be NULL). */
int sdgpu_group_sharded_all_device(sdgpu_ctx *const *ctx, sdgpu_comm *const *comm,
                                   sdgpu_index *const *idx, int ngpu,
                                   const uint64_t *const *d_key, const uint8_t *const *d_has_key,
                                   const uint32_t *const *d_rank, const uint64_t *n,
                                   uint32_t chunk_rows, uint32_t *const *d_rep,
                                   void *const *streams);
/* Sharded grouping + Object write set, with no return leg: each rank writes
 * the write-set entries (as sdgpu_group_link_device: who = rank, or rank |
 * SDGPU_LINKED with obj = the creator's rank) of the keyed rows it OWNS --
 * their cas_id hashes to its shard, whichever rank identified them -- and of
 * its own valid keyless rows.  The union over the ranks is the write set of
 * all rows (a set, mod.rs:189-333), so only the 12-B records cross xGMI.
 * Global ranks in d_rank (required, < 2^31).  d_who / d_obj hold cap
 * entries: -ENOSPC (the peers are unaffected; the lists are not valid) when
 * this rank's owned keyed rows + own keyless rows exceed cap -- up to
 * nranks x n when every row shares one cas_id.  The counted exchange
 * returns it from the call, before any list is written; the padded one
 * finds it on the device (no entry is written past cap) and returns it when
 * the call is resolved (sdgpu_comm_wait).
 * d_counts (device) = [creators, linked, entries].  No Object index (use
 * sdgpu_group_sharded_device with one). */
int sdgpu_group_link_sharded_device(sdgpu_ctx *ctx, sdgpu_comm *comm, const uint64_t *d_key,
                                    const uint8_t *d_has_key, const uint8_t *d_valid,
                                    const uint32_t *d_rank, uint64_t n, uint32_t chunk_rows,
                                    uint32_t *d_who, uint32_t *d_obj, uint64_t cap,
                                    uint32_t *d_counts, void *stream);
/* The same from one process for all ngpu ranks (arrays indexed by rank;
 * d_has_key, d_valid and streams may be NULL). */
int sdgpu_group_link_sharded_all_device(sdgpu_ctx *const *ctx, sdgpu_comm *const *comm, int ngpu,
                                        const uint64_t *const *d_key,
                                        const uint8_t *const *d_has_key,
                                        const uint8_t *const *d_valid,
                                        const uint32_t *const *d_rank, const uint64_t *n,
                                        uint32_t chunk_rows, uint32_t *const *d_who,
                                        uint32_t *const *d_obj, const uint64_t *cap,
                                        uint32_t *const *d_counts, void *const *streams);
/* SURVEY §8(b)'s sdgpu_dedup(ctx[], ngpu, ...): host arrays in rank order,
 * split into ngpu contiguous ranges, grouped across the ngpu contexts
 * (communicators created and destroyed inside). */
int sdgpu_dedup_sharded(sdgpu_ctx *const *ctx, int ngpu, const uint64_t *key,
                        const uint8_t *has_key, uint32_t n, uint32_t chunk_rows, uint32_t *rep);

/* Sharding helpers (single steps of the exchange, for hosts that bring their
 * own collectives, e.g. torch.distributed): shard of a key = top shard_bits
 * bits of mix64(key).  count: h_counts[s] = rows with has_key destined to
 * shard s (host array of 2^shard_bits; synchronises).  partition: packs those
 * rows by shard into d_out_key/d_out_rank (shard s at exclusive prefix of
 * counts) and records each packed row's source index in d_out_pos. */
int sdgpu_shard_count_device(sdgpu_ctx *ctx, const uint64_t *d_key, const uint8_t *d_has_key,
                             uint64_t n, uint32_t shard_bits, uint64_t *h_counts, void *stream);
int sdgpu_shard_partition_device(sdgpu_ctx *ctx, const uint64_t *d_key, const uint8_t *d_has_key,
                                 const uint32_t *d_rank, uint64_t n, uint32_t shard_bits,
                                 uint64_t *d_out_key, uint32_t *d_out_rank, uint32_t *d_out_pos,
                                 void *stream);
/* The send side of the sharded grouping's exchange in one call, with no host
 * synchronisation: the partition of sdgpu_shard_partition_device (one
 * histogram pass) plus d_dest_counts[d] (int64, device) = packed rows destined
 * to rank d, where shard s belongs to rank (s * world) >> shard_bits.  Ranks'
 * segments are contiguous and in rank order in d_out_*; sized n rows (keyless
 * rows are dropped, so the tail is unused).  world <= 64, world <= 2^shard_bits. */
int sdgpu_shard_exchange_device(sdgpu_ctx *ctx, const uint64_t *d_key, const uint8_t *d_has_key,
                                const uint32_t *d_rank, uint64_t n, uint32_t shard_bits,
                                uint32_t world, uint64_t *d_out_key, uint32_t *d_out_rank,
                                uint32_t *d_out_pos, int64_t *d_dest_counts, void *stream);
/* d_dst[d_pos[i]] = d_src[i] for i < n.  With init != 0 every row of d_dst is
 * first set to d_init[r] (or to r when d_init is NULL), so rows without a key
 * keep their own rank (mod.rs:238-239). */
int sdgpu_scatter_rep_device(sdgpu_ctx *ctx, const uint32_t *d_src, const uint32_t *d_pos,
                             uint64_t n, uint32_t *d_dst, uint64_t n_dst, const uint32_t *d_init,
                             int init, void *stream);

/* ---- K7: Object link batch ------------------------------------------------------
 * The write set of identifier_job_step (file_identifier/mod.rs:189-333) for a
 * whole batch of rows, from the grouping's rep[]: rows with rep == own rank
 * create an Object (object::create_many, mod.rs:243-297), the others connect
 * to the Object of row rep (mod.rs:189-225); rows with d_valid[i] == 0 (I/O
 * error, mod.rs:113,127) are in neither list.  Row i has rank d_rank[i]
 * (d_rank NULL: first_rank + i).  Outputs (device): d_create[0..C) creator
 * ranks, d_link_row/d_link_obj[0..L) (row rank, creator rank), both in row
 * order; d_counts[0] = C, d_counts[1] = L.  Each output holds n entries. */
int sdgpu_link_batch_device(sdgpu_ctx *ctx, const uint32_t *d_rep, const uint32_t *d_rank,
                            const uint8_t *d_valid, uint32_t first_rank, uint64_t n,
                            uint32_t *d_create, uint32_t *d_link_row, uint32_t *d_link_obj,
                            uint32_t *d_counts, void *stream);

/* Fused grouping + Object write set (ABI 4): the grouping of
 * sdgpu_group_rows_device and the lists of sdgpu_link_batch_device in one
 * pass, with no rep array in between (the group kernel writes the lists
 * directly, coalesced; file_identifier/mod.rs:189-333).  Rows: d_key[i],
 * d_has_key[i] (NULL = every row keyed), d_valid[i] (NULL = every row valid;
 * a row with valid == 0 must have has_key == 0 and is in no list: it stays an
 * orphan, mod.rs:113,127), rank d_rank[i] or first_rank + i (d_rank NULL),
 * ranks < 2^31.  Output (device), one entry per keyed row and per valid
 * keyless row, n entries each:
 *   d_who[e] = rank                  the row creates an Object
 *   d_who[e] = rank | SDGPU_LINKED   the row connects to the Object created by
 *                                    the row of rank d_obj[e]
 * Keyed rows come first, grouped by an internal hash bucket (creators before
 * linked rows inside a bucket); the valid keyless rows (own Objects,
 * mod.rs:238-239) follow them.  The ORDER of the entries is not
 * part of the contract (the reference's writes are a set; compare as sets).
 * d_counts[0] = creators, [1] = linked rows, [2] = entries (= [0] + [1]). */
#define SDGPU_LINKED 0x80000000u
/* idx (may be NULL): the Object index, as in sdgpu_group_rows_indexed_device:
 * a row whose cas_id already has an Object (registered, or created by an
 * earlier batch) links to it -- obj = SDGPU_REP_EXISTING | handle, or the
 * creator's rank -- and the creators of this batch are added to the index.
 * May synchronise `stream` when the index grows. */
int sdgpu_group_link_device(sdgpu_ctx *ctx, sdgpu_index *idx, const uint64_t *d_key,
                            const uint8_t *d_has_key, const uint8_t *d_valid,
                            const uint32_t *d_rank, uint32_t first_rank, uint64_t n,
                            uint32_t chunk_rows, uint32_t *d_who, uint32_t *d_obj,
                            uint32_t *d_counts, void *stream);

/* ---- downstream consumers of the grouping ---------------
 * Orphan remover (core/src/object/orphan_remover.rs:57-90: Objects with no
 * file_path, `object::file_paths::none`, deleted 512 at a time): d_orphans
 * receives the ids of d_object_ids that no entry of d_fp_object_ids (a
 * file_path's object_id; negative = NULL) references, in list order;
 * d_count[0] = how many.  Object ids must lie in [0, max_object_id]; the
 * context keeps a workspace of max_object_id + 1 bytes (a mark per id). */
int sdgpu_orphan_objects_device(sdgpu_ctx *ctx, const int32_t *d_object_ids, uint64_t n_objects,
                                const int32_t *d_fp_object_ids, uint64_t n_file_paths,
                                uint32_t max_object_id, int32_t *d_orphans, uint32_t *d_count,
                                void *stream);
/* Thumbnail shards (core/src/object/media/thumbnail/shard.rs:4-8: directory =
 * cas_id[0..2] = the first digest byte): d_order = the rows (d_valid[i] != 0,
 * or all when NULL) ordered by shard directory, stable within a directory;
 * d_counts[256] = rows per directory. */
int sdgpu_thumbnail_shards_device(sdgpu_ctx *ctx, const uint8_t *d_cas8, const uint8_t *d_valid,
                                  uint64_t n, uint32_t *d_order, uint32_t *d_counts, void *stream);
/* (ABI 6, additive) Thumbnail remover (core/src/object/thumbnail_remover.rs:
 * 236-367, process_clean_up): which thumbnails on disk does no file_path own
 * any more.  The thumbnails are listed directory by directory: d_thumb_key
 * [n_thumbs] are their cas keys, d_dir_start[0..n_dirs] ascending offsets
 * (directory d owns [start[d], start[d+1]); empty directories are allowed;
 * start[0] = 0, start[n_dirs] = n_thumbs).  The file_paths are n_cols <= 64
 * columns: d_col_key, d_col_has_key and col_rows are HOST arrays of n_cols
 * device pointers / row counts; any col_rows[c] may be 0, d_col_has_key (or
 * any entry of it) may be NULL = every row keyed; a row with has_key == 0
 * owns nothing whatever its key bytes hold.  The set of non-indexed
 * thumbnails is one more column.  d_stale (capacity n_thumbs) receives the
 * positions in the thumbnail list of those no row owns, in list order;
 * d_stale_start[0..n_dirs] their per-directory offsets, d_stale_start[n_dirs]
 * the total: directory d is emptied iff its stale count equals its size.  The
 * same key listed twice gets one answer.  n_thumbs < 2^31 (the table of
 * thumbnail keys in the context's workspace has 2 x n_thumbs slots rounded up
 * to a power of two, 2^31 at the most); -EINVAL on NULL or inconsistent
 * arguments.  Asynchronous on `stream`, no synchronisation.
 * One GPU: a sharded library runs the call on every share's columns and ORs
 * the answers (a thumbnail is stale when it is stale on every share). */
int sdgpu_stale_thumbnails_device(sdgpu_ctx *ctx, const uint64_t *d_thumb_key, uint64_t n_thumbs,
                                  const uint32_t *d_dir_start, uint32_t n_dirs,
                                  const uint64_t *const *d_col_key,
                                  const uint8_t *const *d_col_has_key, const uint64_t *col_rows,
                                  uint32_t n_cols, uint32_t *d_stale, uint32_t *d_stale_start,
                                  void *stream);
/* (ABI 6, additive) The same on host arrays (what the Rust actor calls with the
 * columns it fetched from the databases; col_key / col_has_key hold host
 * pointers): copy in, run, copy out; returns when done.  dir_start is checked
 * (-EINVAL unless it ascends from 0 to n_thumbs). */
int sdgpu_stale_thumbnails(sdgpu_ctx *ctx, const uint64_t *thumb_key, uint64_t n_thumbs,
                           const uint32_t *dir_start, uint32_t n_dirs,
                           const uint64_t *const *col_key, const uint8_t *const *col_has_key,
                           const uint64_t *col_rows, uint32_t n_cols, uint32_t *stale,
                           uint32_t *stale_start);
/* (ABI 6, additive) Thumbnailer work list (core/src/object/media/thumbnail/
 * mod.rs:204-359, process): which file_paths still need a thumbnail.  The
 * reference builds <base>/<cas_id[0..2]>/<cas_id>.webp for every row of a step
 * (:254-256), stats it (:273), skips the row when the file exists and
 * `regenerate` is off (:301-307) and generates otherwise (:327-343), in steps
 * of 10 rows (media_processor/job.rs:34,151; shallow.rs:31,105) of one query
 * (media_processor/mod.rs:74-116); the explorer stats the same path per item
 * (api/search.rs:540-547, :686-695; library/library.rs:122-130
 * thumbnail_exists).  Here: d_thumb_key[n_thumbs] = the cas keys of the
 * thumbnails on disk (duplicates allowed); one column of file_path rows in
 * ascending id order, d_key[n], d_has_key[n] (NULL = every row keyed),
 * d_eligible[n] (NULL = every row eligible; the caller's WHERE clause:
 * location, extension list, sub-path).  flags: 0 or SDGPU_THUMBS_REGENERATE.
 *   present[i] = 1 iff has_key[i] != 0 and key[i] is a thumbnail key (whatever
 *     eligible[i] is: thumbnail_exists of the row's cas_id), else 0;
 *   row i is a candidate iff has_key[i] != 0, eligible[i] != 0 and
 *     (present[i] == 0 or REGENERATE);
 *   row i is a work row iff it is a candidate and no candidate j < i has
 *     key[j] == key[i]; rows that are no candidates shadow nothing.
 * d_work[0 .. W) = the work rows ordered by shard directory (key & 0xFF, the
 * first cas byte, shard.rs:4-8), ascending inside a directory; nothing is
 * written past W (capacity n).  d_dir_start[0..256] = exclusive offsets into
 * d_work, d_dir_start[256] = W.  d_stats[4] = keyed rows with present == 1;
 * keyed and eligible rows; those of them with present == 1; W.  d_present
 * [n] may be NULL.  The keys 0 and ~0 are ordinary keys on both sides.
 * Presence only (the explorer's call): d_work and d_dir_start both NULL --
 * d_present and d_stats[0] alone, no grouping runs, d_stats[1..3] = 0.
 * n == 0: zeros in d_dir_start and d_stats; n_thumbs == 0: nothing is present.
 * Deviation: the reference generates two rows of one step that share a cas_id
 * twice (the same file written twice) and counts both as created; here every
 * distinct cas_id is a work row once, the files on disk afterwards are the same
 * set, and created / skipped differ by exactly the number of in-step copies.
 * -EINVAL: d_present and d_work both NULL, exactly one of d_work / d_dir_start
 * NULL, NULL d_stats, NULL d_key with n > 0, NULL d_thumb_key with n_thumbs >
 * 0, any other flag bit, n >= 2^31 or n_thumbs >= 2^31.  Asynchronous on
 * `stream`, no synchronisation. */
#define SDGPU_THUMBS_REGENERATE 1u
int sdgpu_thumbnail_worklist_device(sdgpu_ctx *ctx, const uint64_t *d_thumb_key,
                                    uint64_t n_thumbs, const uint64_t *d_key,
                                    const uint8_t *d_has_key, const uint8_t *d_eligible,
                                    uint64_t n, uint32_t flags, uint8_t *d_present,
                                    uint32_t *d_work, uint32_t *d_dir_start, uint32_t *d_stats,
                                    void *stream);
/* (ABI 6, additive) The same on host arrays (what the media processor calls
 * with the rows it fetched): copy in, run, copy out; returns when done.  Only
 * dir_start[256] entries of work travel back. */
int sdgpu_thumbnail_worklist(sdgpu_ctx *ctx, const uint64_t *thumb_key, uint64_t n_thumbs,
                             const uint64_t *key, const uint8_t *has_key,
                             const uint8_t *eligible, uint64_t n, uint32_t flags,
                             uint8_t *present, uint32_t *work, uint32_t *dir_start,
                             uint32_t *stats);
/* (ABI 6, additive) Indexer rescan diff (core/src/location/indexer/walk.rs:
 * 309-381 filter_existing_paths, :624-636 the per-directory to_remove query;
 * indexer/mod.rs:305-331 file_paths_db_fetcher_fn, :338-388
 * to_remove_db_fetcher_fn): which walked entries are new (to_create), which
 * changed behind the library's back (to_update; the indexer then clears their
 * cas_id and Object, indexer/mod.rs:207-215) and which file_path rows are gone
 * from disk (to_remove), for ONE location in one call.  Walking, the indexer
 * rules and the database writes stay with the caller.
 * A 64-bit key stands for a row's unique tuple (materialized_path, name,
 * extension), a second one for a directory's materialized_path_for_children()
 * (file_path_helper/isolated_file_path_data.rs:150-158); only equality of keys
 * is used, and the caller makes the answer exact by comparing the strings of
 * every matched pair.
 *   Walked entries (walk.rs's indexed_paths: accepted by the rules, ancestors
 *   included): d_w_key[n_w]; d_w_flags[n_w] (NULL = all 0), bit 0 is_dir, bit 1
 *   SDGPU_IDX_ANCESTOR = the entry was pushed as an ancestor from a deeper
 *   directory (walk.rs:560-617) and was in no listing of its own parent;
 *   d_w_meta[n_w][3] = inode, device, modified_at (int64 ns since the epoch).
 *   Walked directories: d_wd_key[n_wd], the children-path keys of the
 *   directories whose listing was read; duplicates allowed.
 *   file_path rows of the location in ascending id order: d_r_key[n_r];
 *   d_r_dirkey[n_r] = the key of the row's own materialized_path; d_r_flags
 *   [n_r] (NULL = all 0), bit 0 is_dir, bit 1 SDGPU_IDX_NO_METADATA = inode,
 *   device or date_modified is NULL in the row (walk.rs:349-354); d_r_meta
 *   [n_r][3] laid out as d_w_meta.
 * For entry i let j0 = the lowest row with r_key == w_key[i]:
 *   d_match[i] = j0, or SDGPU_IDX_MISS when no row has the key (written
 *     whatever is_dir says, so the caller can check the pair's strings);
 *   d_state[i] = 0 CREATE: no such row;
 *                3 KIND_CHANGED: is_dir of row j0 differs from the entry's --
 *                  the reference's HashMap is keyed by IsolatedFilePathData,
 *                  whose Hash / Eq include is_dir (isolated_file_path_data.rs:
 *                  25-38), so the entry misses it and is created;
 *                2 UPDATE: same is_dir, row j0 has metadata, and inode differs,
 *                  or device differs, or (int64)(w_mtime - r_mtime) > 1 000 000
 *                  (one-sided, strict, signed, walk.rs:360-364: a row newer than
 *                  the disk is left alone; the difference is taken in 64-bit
 *                  two's complement);
 *                1 UNCHANGED: otherwise, a matched NO_METADATA row included.
 *   d_create = the entries of state 0 or 3, d_update those of state 2, both
 *     ascending entry indices (capacity n_w each);
 *   d_remove = ascending row indices j (capacity n_r) with r_dirkey[j] among
 *     d_wd_key and no entry i with w_key[i] == r_key[j] whose ANCESTOR bit is
 *     clear.  is_dir plays no part (the reference's found ids come from the
 *     4-term query): a file replaced by a directory of the same name is created
 *     (state 3) and NOT removed, as in the reference.  Rows of directories that
 *     were not walked are never removed.
 *   d_counts[4] = len(create), len(update), len(remove), entries of state 3.
 * Nothing is written past the three lengths.  Duplicated keys (a caller error
 * under the schema) stay defined: all rows of one key are spared or removed
 * together, j0 answers for the key, every walked copy gets its own answer.
 * The keys 0 and ~0 are ordinary keys on every side.  Any count may be 0.
 * -EINVAL: a NULL required pointer with a non-zero count (d_match, d_state,
 * d_create, d_update with n_w > 0; d_remove with n_r > 0; d_counts with any
 * count > 0), a count >= 2^31.  The table of row keys in the context's
 * workspace has 2 x n_r slots rounded up to a power of two, 2^31 at the most.
 * Asynchronous on `stream`, no synchronisation. */
#define SDGPU_IDX_ANCESTOR 2u
#define SDGPU_IDX_NO_METADATA 2u
#define SDGPU_IDX_MISS 0xFFFFFFFFu
int sdgpu_indexer_diff_device(sdgpu_ctx *ctx, const uint64_t *d_w_key, const uint8_t *d_w_flags,
                              const uint64_t *d_w_meta, uint64_t n_w, const uint64_t *d_wd_key,
                              uint64_t n_wd, const uint64_t *d_r_key, const uint64_t *d_r_dirkey,
                              const uint8_t *d_r_flags, const uint64_t *d_r_meta, uint64_t n_r,
                              uint32_t *d_match, uint8_t *d_state, uint32_t *d_create,
                              uint32_t *d_update, uint32_t *d_remove, uint32_t *d_counts,
                              void *stream);
/* (ABI 6, additive) The same on host arrays (what the indexer job calls with
 * the rows it fetched and the entries it walked): copy in, run, copy out;
 * returns when done.  Only counts[0..2] entries of the three lists travel
 * back. */
int sdgpu_indexer_diff(sdgpu_ctx *ctx, const uint64_t *w_key, const uint8_t *w_flags,
                       const uint64_t *w_meta, uint64_t n_w, const uint64_t *wd_key,
                       uint64_t n_wd, const uint64_t *r_key, const uint64_t *r_dirkey,
                       const uint8_t *r_flags, const uint64_t *r_meta, uint64_t n_r,
                       uint32_t *matched, uint8_t *state, uint32_t *create, uint32_t *update,
                       uint32_t *remove, uint32_t *counts);

/* (ABI 6, additive) Recursive directory sizes of ONE location in one call.
 * The reference stores FilePathMetadata.size_in_bytes in
 * file_path.size_in_bytes_bytes for every entry (core/src/location/indexer/
 * mod.rs:126-136, 215-225) -- for a directory the size of its inode, which says
 * nothing of the contents -- and orders and shows by that column
 * (api/search.rs:85, api/locations.rs:66-100).  This call sums the files below
 * every directory; storing the result is the caller's choice.
 *   file_path rows of the location in ascending id order: d_r_dirkey[n_r] = the
 *   key of the row's own materialized_path (as in sdgpu_indexer_diff);
 *   d_r_selfkey[n_r] = for a directory row the key of its
 *   materialized_path_for_children(), not read for a file row; d_r_flags[n_r]
 *   (NULL = no directory rows; d_r_selfkey is then not read), bit 0 is_dir;
 *   d_r_size[n_r] = size_in_bytes of a file row, not read for a directory row.
 * Only equality of keys is used; the caller makes the answer exact by comparing
 * the strings of every pair (i, d_parent[i]).
 *   d_parent[i] = the lowest directory row j with r_selfkey[j] == r_dirkey[i],
 *     or SDGPU_IDX_MISS when there is none (the location's top-level rows, and
 *     rows whose directory row is absent).  Of two directory rows with one self
 *     key the lowest owns the children; the other has none.
 *   d_total[i] = r_size[i] for a file row; for a directory row the sum of r_size
 *     over every file row below it, transitively through d_parent, modulo 2^64
 *     (0 for an empty directory).
 *   d_files[i] (may be NULL) = the file rows below a directory row; 0 for a file
 *     row.
 *   A directory row on a cycle of d_parent (a row that is its own parent, say: a
 *     bad key or a collision) is unresolved: d_total = SDGPU_SIZE_UNRESOLVED,
 *     d_files = 0xFFFFFFFF.  Every other directory row gets its exact answer; a
 *     subtree that hangs below a cycle has its own totals, the cycle absorbs
 *     them.
 *   d_counts[4] = directory rows, directory rows resolved, rows with d_parent ==
 *     SDGPU_IDX_MISS, the sum of d_total over those rows modulo 2^64 (the
 *     location's size).  d_counts[1] < d_counts[0]: re-key with another salt.
 * Every output is defined for every input and deterministic.  The keys 0 and
 * ~0 are ordinary keys.  n_r == 0 is valid: the four counts are 0.
 * -EINVAL: ctx or d_counts NULL; with n_r > 0 a NULL d_r_dirkey, d_r_size,
 * d_parent or d_total, or d_r_flags without d_r_selfkey.  -E2BIG: n_r > 2^31.
 * Both are decided before any device work.  The table of self keys in the
 * context's workspace has 2 x (directory rows) slots rounded up to a power of
 * two (at least 1024), 12 bytes a slot.  The device variant learns the number of
 * directory rows on the device only, so it RESERVES the workspace for the
 * worst case, every row a directory: with d_r_flags given about 12 bytes x (2 x
 * n_r rounded up to a power of two) + 8 n_r (+ 4 n_r without d_files), of which
 * the kernels touch the front part that the real number needs -- at 12.5 M rows
 * 384 MiB + 100 MB reserved, 24 MiB of table touched for 1 M directories.  The
 * host-array variant counts the flags and reserves exactly.  Asynchronous on
 * `stream`, no synchronisation. */
#define SDGPU_SIZE_UNRESOLVED 0xFFFFFFFFFFFFFFFFull
int sdgpu_dir_sizes_device(sdgpu_ctx *ctx, const uint64_t *d_r_dirkey,
                           const uint64_t *d_r_selfkey, const uint8_t *d_r_flags,
                           const uint64_t *d_r_size, uint64_t n_r, uint32_t *d_parent,
                           uint64_t *d_total, uint32_t *d_files, uint64_t *d_counts,
                           void *stream);
/* (ABI 6, additive) The same on host arrays: copy in, run, copy out; returns
 * when done. */
int sdgpu_dir_sizes(sdgpu_ctx *ctx, const uint64_t *r_dirkey, const uint64_t *r_selfkey,
                    const uint8_t *r_flags, const uint64_t *r_size, uint64_t n_r,
                    uint32_t *parent, uint64_t *total, uint32_t *files, uint64_t *counts);

/* ---- sync ingest: which CRDT operations apply (ABI 6, additive) -----------------
 * The receiving half of library sync, core/crates/sync/src/ingest.rs.
 * receive_crdt_operation (ingest.rs:114-160) handles one op at a time, strictly
 * in page order (ingest.rs:67-71; pages of 1000 ops, core/src/p2p/sync/mod.rs:
 * 403-431).  For each op compare_message (ingest.rs:188-233) finds the newest
 * op of shared_operation / relation_operation (core/prisma/schema.prisma:21-53)
 * with timestamp >= t and the op's (model, record_id, kind) or (relation,
 * item_id, kind) -- group_id plays no part (ingest.rs:213-220); kind is "c",
 * "u:<field>" or "d" (crates/sync/src/crdt.rs:9-23,34-36,67-69) -- and the op is
 * old exactly when one exists and its timestamp != t.  With L(k) the largest
 * logged timestamp of key k in SIGNED int64 order (an NTP64 stored
 * `as_u64() as i64`, compared as SQLite compares the BigInt column):
 *     old  <=>  L(k) > t;   an equal timestamp is not old (a re-delivered op is
 *     applied again).
 * An op that is not old is applied and logged (apply_op, ingest.rs:162-186), so
 * later ops of the page see it; an old op lies below the running maximum.  Hence
 *     apply[i] = ( t[i] >= max( L(key[i]), max{ t[j] : j < i, key[j] == key[i] } ) )
 * Old or not, the instance's clock becomes max(clock or t, t) in UNSIGNED NTP64
 * order (ingest.rs:119-126,151).  An absent L equals INT64_MIN and an absent
 * clock 0; neither sentinel changes any answer.  get_ops (manager.rs:130-199),
 * the writes of apply_op, the HLC and the transport stay with the caller.
 *
 * A key is 64 bits of BLAKE3 of the tuple (the reference compares the strings);
 * a tag is a second, independent 64-bit hash of the same tuple (a caller that
 * has none passes the key).  The thread that enters a key into the log stores
 * its tag; every other op of that key, in this call or any later one, compares
 * its tag with the stored one, and the disagreements are counted.  A non-zero
 * count means two tuples share a key and the answers for them are not the
 * reference's: the caller re-keys with another salt and reloads the log.  The
 * case is detected, not repaired.
 *
 * sdgpu_oplog: key -> newest logged timestamp; lives as long as the library.
 * Open addressing, 32-byte slots, load <= 1/2, at most 2^31 slots (-ENOSPC
 * beyond).  The handle belongs to `ctx` and must be destroyed before it. */
typedef struct sdgpu_oplog sdgpu_oplog;
/* (ABI 6, additive) capacity_hint: keys expected (<= 2^30; the log grows). */
int sdgpu_oplog_create(sdgpu_ctx *ctx, uint64_t capacity_hint, sdgpu_oplog **out);
/* (ABI 6, additive) */
int sdgpu_oplog_destroy(sdgpu_oplog *log);
/* (ABI 6, additive) Forgets every key; the capacity stays. */
int sdgpu_oplog_clear(sdgpu_oplog *log, void *stream);
/* (ABI 6, additive) out = {keys stored, capacity in slots}; synchronises. */
int sdgpu_oplog_stats(sdgpu_oplog *log, uint64_t out[2]);
/* (ABI 6, additive) Loads existing op-log rows (what compare_message's
 * find_first would scan, ingest.rs:188-233): L(key) = max(L(key), ts) in signed
 * order; the order of the rows does not matter.  d_collisions (device, may be
 * NULL) = the rows whose tag is not the one stored with their key.  -EINVAL: a
 * NULL d_key, d_tag or d_ts with n > 0, n >= 2^31.  May synchronise `stream`
 * when the table grows; otherwise asynchronous. */
int sdgpu_oplog_add_device(sdgpu_oplog *log, const uint64_t *d_key, const uint64_t *d_tag,
                           const int64_t *d_ts, uint64_t n, uint32_t *d_collisions, void *stream);
/* (ABI 6, additive) d_ts[i] = L(d_key[i]) and d_found[i] = 1 (ingest.rs:188-233
 * asks for the same row); for a key that is absent or holds no timestamp yet
 * INT64_MIN and 0 -- a logged op at INT64_MIN reads the same way, which changes
 * no decision.  A pure read: no growth, asynchronous. */
int sdgpu_oplog_latest_device(sdgpu_oplog *log, const uint64_t *d_key, uint64_t n,
                              int64_t *d_ts, uint8_t *d_found, void *stream);
/* (ABI 6, additive) One page of ops in arrival order (ingest.rs:114-160, the
 * rule above):
 *   d_apply[i] = 1 when op i applies, else 0;
 *   d_applied  = the ascending indices with apply == 1 (capacity n);
 *   d_winner   = the ascending indices of the highest-index applied op of every
 *                key that has one -- the only ops whose value survives in the
 *                row (capacity n);
 *   d_counts[4] = applied, winners, keys new to the log, tag disagreements.
 * Nothing is written past the two list lengths.  Afterwards L(k) includes every
 * applied op (ingest.rs:162-186).  SDGPU_INGEST_NO_COMMIT: the same decisions,
 * in-page visibility included, but no timestamp in the log changes (the page's
 * keys may still be entered, with no timestamp); the caller commits later with
 * sdgpu_oplog_add_device.
 *   d_clock[d_instance[i]] = max_u64(old, (uint64_t)d_ts[i]) for every op
 * (ingest.rs:119-126,151); an index >= n_instances updates nothing; d_instance
 * and d_clock may both be NULL with n_instances == 0.
 * The keys 0 and ~0 are ordinary keys.  n == 0 zeroes the counts.  -EINVAL: a
 * NULL required pointer with n > 0, n >= 2^31, unknown flag bits, exactly one of
 * d_instance / d_clock given.  May synchronise `stream` when the table grows, as
 * sdgpu_index_* does; otherwise asynchronous, no synchronisation. */
#define SDGPU_INGEST_NO_COMMIT 1u
int sdgpu_sync_ingest_device(sdgpu_oplog *log, const uint64_t *d_key, const uint64_t *d_tag,
                             const int64_t *d_ts, const uint32_t *d_instance, uint64_t n,
                             uint64_t *d_clock, uint32_t n_instances, uint32_t flags,
                             uint8_t *d_apply, uint32_t *d_applied, uint32_t *d_winner,
                             uint32_t *d_counts, void *stream);
/* (ABI 6, additive) The same on host arrays (what the actor's Ingesting state,
 * ingest.rs:67-71, calls with a received page): copy in, run, copy out; returns
 * when done.  Only counts[0] / counts[1] entries of the two lists travel back.
 * n == 0 is decided without a device. */
int sdgpu_sync_ingest(sdgpu_oplog *log, const uint64_t *key, const uint64_t *tag,
                      const int64_t *ts, const uint32_t *instance, uint64_t n, uint64_t *clock,
                      uint32_t n_instances, uint32_t flags, uint8_t *apply, uint32_t *applied,
                      uint32_t *winner, uint32_t *counts);

/* ---- explorer: one search page (ABI 6, additive) -------------------------------
 * search.paths (core/src/api/search.rs:393-562), the query behind every folder
 * view, category view and infinite scroll, over columns the caller keeps on the
 * device: the WHERE clause over file_path and its Object (:127-187, :302-324),
 * ORDER BY is_dir DESC, <field>, id (:429-431, :436-445, :477-478, :526-527), a
 * keyset cursor (:446-528) or an offset (:439-445), take <= 100 (:421).  The
 * count calls (pathsCount :563-582, objectsCount) are the same filter with
 * take == 0; search.objects (:583-708) is the same call with the Object columns
 * passed as the rows.  The per-item thumbnail_exists (:540-547) is the presence
 * mode of the thumbnailer work list above.
 *
 * The three structs are plain host structs, read when the call is made; their
 * array members are device pointers for the _device call, host pointers for the
 * host call.  A column the query does not use may be NULL.
 *
 * Rows: one table's file_path rows in ascending id order; row index stands for
 * id, as in the thumbnailer.  i64 values lie in (-2^62, 2^62), SDGPU_SEARCH_NULL
 * is SQL NULL (nanosecond dates stay inside the range until the year 2116).
 *
 * Semantics: SQLite's three-valued logic, as the reference's Prisma client runs
 * it -- a comparison with a NULL column value is false.
 * Filter.  Row i matches iff eligible[i] != 0 (NULL pointer: every row; the
 * caller's remaining WHERE terms, e.g. name contains, :165-169) and every term
 * of `use` holds:
 *   LOCATION      location[i] = location (:171)   EXTENSION  ext[i] = ext (:172)
 *   CREATED_FROM  date_created[i] >= created_from (:173)
 *   CREATED_TO    date_created[i] <= created_to (:174)
 *   DIR           dir_key[i] = dir_key (materialized_path equals, :175-177)
 * and on the row's Object o = object[i] (object::is(params), :178-182; any of
 * these terms, or the flag NEEDS_OBJECT, fails a row with object[i] < 0 -- the
 * default `hidden: Exclude` alone switches that on, :273-283):
 *   HIDDEN_EXCLUDE  not (hidden is true): flags[o] bit 2 clear (:276-279)
 *   FAVORITE        operand 1: flags[o] bit 0 set; operand 0: bits 0 (true) and
 *                   1 (NULL) both clear (:310)
 *   KIND            kind[o] not NULL and bit kind[o] of kind_mask set (:313;
 *                   library/cat.rs:62-75)
 *   TAGS            some pair (tag_obj, tag_tag) = (o, t) with t among
 *                   tags[0..n_tags) (:314-319); duplicate pairs allowed
 *   ACCESSED_EQ v   date_accessed[o] = v, or IS NULL when v is SDGPU_SEARCH_NULL
 *   ACCESSED_NE v   date_accessed[o] <> v (false for a NULL column), or IS NOT
 *                   NULL when v is SDGPU_SEARCH_NULL (:311-312, cat.rs:64)
 * Candidates.  A matching row is a candidate iff it passes FILES_ONLY (bit 0 of
 * flags[i] clear, :453-455) and the cursor predicate: true without CURSOR; with
 * CURSOR and no order key, i >= cursor_row (:483-485); with an order key v and
 * cursor_key c, a NULL v fails, and otherwise
 *   ascending   v > c, or (without CURSOR_STRICT) v == c and i >= cursor_row;
 *   descending  v < c, or (without CURSOR_STRICT) v == c and i <  cursor_row
 * (:463-475).  The caller turns the cursor's id into cursor_row: the number of
 * rows with id <= it when ascending, with id < it when descending.  The order
 * key is order_key[i], or with ORDER_BY_OBJECT objects->order_key[object[i]]
 * (NULL for a row with no Object); a NULL order_key pointer = no order field.
 * Order.  Directories first under GROUP_DIRS, in both directions (:429-431);
 * then the order key, NULL lowest (first ascending, last descending, SQLite's
 * rule); then ascending row index, always.
 * Outputs.  d_page[0..P) = the candidates of ranks [offset, offset + take) in
 * that order, nothing is written past P; d_counts[4] = matching rows
 * (pathsCount), candidates, P = min(take, max(0, candidates - offset)),
 * directories among the matching rows (0 when rows->flags is NULL).  take == 0
 * is the count call, d_page may then be NULL.
 * Kept from the reference: the cursor predicate applies to directories and
 * files alike (:453-479); descending ties compare id < while the order stays id
 * ascending (:472, :526-527); the Object-field cursors have no tie arm
 * (:497-515) -- CURSOR_STRICT; NULL-keyed rows are never reached through a
 * cursor.  Deviation: where the reference gives no final id order (OrderOnly
 * and Offset, :436-445) SQLite's tie order is unspecified; here ties are
 * always ascending id, one of the orders SQLite may return.
 * Exactness: dir_key is a 64-bit stand-in (the indexer's r_dirkey); the caller
 * string-checks the at most SDGPU_SEARCH_MAX_TAKE returned rows, as the
 * indexer's caller checks its matched pairs.
 * The selection is exact and sorts at most SDGPU_SEARCH_SELECT_FINAL records,
 * whatever offset is.
 * -EINVAL: NULL ctx, rows, query or d_counts; take > SDGPU_SEARCH_MAX_TAKE;
 * d_page NULL with take > 0; CURSOR together with a non-zero offset;
 * CURSOR_STRICT without CURSOR; ORDER_BY_OBJECT without objects; n_tags > 32;
 * an unknown bit in `use` or `flags`; a column the query uses that is NULL
 * (rows->flags with GROUP_DIRS or FILES_ONLY; rows->object with any Object
 * term, NEEDS_OBJECT or ORDER_BY_OBJECT; `objects` and its column with an
 * Object term; the pair arrays with TAGS and n_pairs > 0); n, m or n_pairs >=
 * 2^31; negative offset.  n == 0: zeros in d_counts.  Asynchronous on
 * `stream`, no synchronisation. */
#define SDGPU_SEARCH_MAX_TAKE 256u
#define SDGPU_SEARCH_SELECT_FINAL 3840u
#define SDGPU_SEARCH_NULL (-(INT64_C(1) << 62))
#define SDGPU_SEARCH_USE_LOCATION 0x1u
#define SDGPU_SEARCH_USE_EXTENSION 0x2u
#define SDGPU_SEARCH_USE_CREATED_FROM 0x4u
#define SDGPU_SEARCH_USE_CREATED_TO 0x8u
#define SDGPU_SEARCH_USE_DIR 0x10u
#define SDGPU_SEARCH_USE_FAVORITE 0x20u
#define SDGPU_SEARCH_USE_HIDDEN_EXCLUDE 0x40u
#define SDGPU_SEARCH_USE_KIND 0x80u
#define SDGPU_SEARCH_USE_TAGS 0x100u
#define SDGPU_SEARCH_USE_ACCESSED_EQ 0x200u
#define SDGPU_SEARCH_USE_ACCESSED_NE 0x400u
#define SDGPU_SEARCH_DESC 0x1u
#define SDGPU_SEARCH_GROUP_DIRS 0x2u
#define SDGPU_SEARCH_FILES_ONLY 0x4u
#define SDGPU_SEARCH_CURSOR 0x8u
#define SDGPU_SEARCH_CURSOR_STRICT 0x10u
#define SDGPU_SEARCH_ORDER_BY_OBJECT 0x20u
#define SDGPU_SEARCH_NEEDS_OBJECT 0x40u
typedef struct sdgpu_search_rows_t {
  uint64_t n;
  const int32_t *location;     /* [n] -1 = NULL */
  const uint16_t *ext;         /* [n] id in the caller's dictionary of extension strings,
                                  0xFFFF = NULL */
  const uint64_t *dir_key;     /* [n] key of the row's materialized_path (r_dirkey) */
  const uint8_t *flags;        /* [n] bit 0 = is_dir is true */
  const int64_t *date_created; /* [n] */
  const int32_t *object;       /* [n] index into the Object columns, -1 = no Object */
  const uint8_t *eligible;     /* [n] NULL = every row */
  const int64_t *order_key;    /* [n] the column the query orders by: a date, the size, a
                                  rank of the name under the database's collation */
} sdgpu_search_rows_t;
typedef struct sdgpu_search_objects_t {
  uint64_t m;
  const int32_t *kind;          /* [m] -1 = NULL */
  const uint8_t *flags;         /* [m] bit 0 favorite is true, bit 1 favorite is NULL,
                                   bit 2 hidden is true */
  const int64_t *date_accessed; /* [m] */
  const int64_t *order_key;     /* [m] */
  const int32_t *tag_obj;       /* [n_pairs] the tag_on_object pairs */
  const int32_t *tag_tag;       /* [n_pairs] */
  uint64_t n_pairs;
} sdgpu_search_objects_t;
typedef struct sdgpu_search_query_t {
  uint32_t use;      /* SDGPU_SEARCH_USE_* */
  uint32_t flags;    /* SDGPU_SEARCH_DESC ... _NEEDS_OBJECT */
  int32_t location;
  uint16_t ext;
  uint16_t favorite; /* 0 / 1 */
  uint64_t dir_key;
  int64_t created_from;
  int64_t created_to;
  uint32_t kind_mask; /* bit = ObjectKind value */
  uint32_t n_tags;
  int32_t tags[32];
  int64_t accessed_eq;
  int64_t accessed_ne;
  int64_t cursor_key;
  int64_t cursor_row;
  int64_t offset;
  uint32_t take;
  uint32_t reserved; /* 0 */
} sdgpu_search_query_t;
int sdgpu_search_page_device(sdgpu_ctx *ctx, const sdgpu_search_rows_t *rows,
                             const sdgpu_search_objects_t *objects,
                             const sdgpu_search_query_t *query, uint32_t *d_page,
                             uint32_t *d_counts, void *stream);
/* (ABI 6, additive) The same on host arrays (what the explorer's rspc handler
 * calls with columns it holds in memory): copy in the columns the query uses,
 * run, copy back counts and only counts[2] entries of page; returns when done.
 * n == 0 is decided without a device. */
int sdgpu_search_page(sdgpu_ctx *ctx, const sdgpu_search_rows_t *rows,
                      const sdgpu_search_objects_t *objects, const sdgpu_search_query_t *query,
                      uint32_t *page, uint32_t *counts);

/* ---- synthetic corpora (bench / tests; same content function as oracle/) ---- */
int sdgpu_synth_cas_arena_device(sdgpu_ctx *ctx, const uint64_t *d_sizes, const uint64_t *d_seeds,
                                 const uint64_t *d_off, uint32_t n, uint8_t *d_arena, void *stream);
int sdgpu_synth_file_device(sdgpu_ctx *ctx, uint64_t seed, uint64_t offset, uint64_t len,
                            uint8_t *d_out, void *stream);
/* Dedup corpus (BASELINE config 4 shape): global rows [first_rank, first_rank+n)
 * of a table of total_rows rows whose keys are a random permutation of
 * `distinct` distinct keys plus (total_rows - distinct) duplicates of them;
 * one row in 1000 has no key.  Writes key, has_key and rank (= global row). */
int sdgpu_synth_dedup_rows_device(sdgpu_ctx *ctx, uint64_t seed, uint64_t total_rows,
                                  uint64_t distinct, uint64_t first_rank, uint64_t n,
                                  uint64_t *d_key, uint8_t *d_has_key, uint32_t *d_rank,
                                  void *stream);

/* Config-5 run (bench): step `step` of a run over one pinned pool of files --
 * rows with d_vary[i] != 0 stand for files with new content (key' =
 * mix64(key ^ step * 0x9E3779B97F4A7C15), a bijection); the others are the
 * same files in every step.  step 0 leaves every key unchanged. */
int sdgpu_synth_vary_keys_device(sdgpu_ctx *ctx, uint64_t *d_key, const uint8_t *d_vary,
                                 uint64_t n, uint64_t step, void *stream);

/* ---- instrumentation (bench / profiling) ---------------------------------------
 * With timing enabled every main kernel launched through ctx is bracketed by
 * HIP events on its own stream; sdgpu_timing_read returns, per kernel name
 * (e.g. "cas_chunks", "tree_leaves", "bucket_group"), the accumulated device
 * milliseconds and launch count (-ENOENT past the last entry). */
int sdgpu_set_timing(sdgpu_ctx *ctx, int enable);
int sdgpu_timing_reset(sdgpu_ctx *ctx);
int sdgpu_timing_read(sdgpu_ctx *ctx, uint32_t idx, char name[32], double *total_ms,
                      uint64_t *launches);
/* Measured int32 VALU issue rate (lane-ops/s) of a BLAKE3-G-shaped
 * add3/xor/alignbit stream at full occupancy: the VALU roofline's peak. */
int sdgpu_valu_probe(sdgpu_ctx *ctx, double *lane_ops_per_s);
/* Same for one instruction class: 0 the G mix above, 1 v_xor_b32, 2 v_add3_u32,
 * 3 v_alignbit_b32, 4 v_add_u32; 5 = whole BLAKE3 compressions with everything
 * in registers (680 VALU each): the attainable roof of K1/K2's stream. */
int sdgpu_valu_probe_kind(sdgpu_ctx *ctx, int kind, double *lane_ops_per_s);
/* Latency breakdown of the last service request (sdgpu_latency_service) in
 * microseconds: [0] message copied into LDS, [1] hashed and digest written
 * (device wall clock), [2] host: post -> answer seen, [3] host: the file read
 * (the last two for sdgpu_generate_cas_id). */
int sdgpu_latency_service_diag(sdgpu_ctx *ctx, double out_us[4]);

#ifdef __cplusplus
}
#endif

#endif /* SDGPU_H */

/*
 * genome_amd.h — C-ABI of the MI355X-native k-mer hashtable + de Bruijn graph-build core.
 *
 * This is the drop-in boundary for the data-parallel hot path of winger/genome
 * (S/ = /root/reference/src/main/scala/ru/ifmo/genome/).  Plain pointers and sizes only; no torch
 * types.  Each entry point names the reference interface it replaces.  The Scala-side binding a
 * maintainer would add (JNI stub + `HipDNAMap extends DNAMap[Int]`) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - Every function returns a gk_status (0 = ok, <0 = error); the message of the last error of a
 *     context is available through gk_last_error().  Nothing aborts.  (Reference: `assert` =>
 *     AssertionError on wrong key length, S/ds/ArrayDNAMap.scala:182; failures surface via Future.)
 *   - Handles are opaque, created/destroyed by the caller and EXTERNALLY SYNCHRONISED: one call at
 *     a time per handle, from any thread (reference: an ArrayDNAMap is confined to its actor).
 *   - Calls are synchronous on return.  Host input buffers are borrowed for the duration of the
 *     call; export buffers are caller-allocated with a capacity and an out-count.
 *   - `_dev` variants take DEVICE pointers (hipMalloc'ed by the caller, e.g. a torch tensor's
 *     data_ptr()) valid on the context's device.
 *   - k-mers cross the ABI as little-endian uint64 lo[,hi] in the reference bit layout: base i at
 *     bits 2i of lo (i<32) / 2(i-32) of hi, codes A=0 G=1 C=2 T=3, unused high bits zero
 *     (S/dna/DNASeq.scala:74-215, S/dna/Base.scala:13-19).  `hi` arrays may be NULL when k<=32.
 *     Counts are int32 (the reference's DNAMap[Int]).
 *   - Supported k: 2..31 and 34..64, as in the reference: k=32/33 are broken in the reference itself
 *      and k>64 takes its un-specialised ArrayDNASeq path: GK_E_UNSUPPORTED_K.
 *   - There is no CPU fallback: without a gfx950 device every compute call fails with
 *     GK_E_NODEVICE / GK_E_HIP.
 *   - This is everything a host binds.  The library's test hooks (A/B switches of the kernels, failure injection, a loopback
 *     transport that runs several ranks on one GPU) are NOT in libgenome_amd.so: they live in the test build,
 *     libgenome_amd_test.so, behind include/genome_amd_test.h.
 */
#ifndef GENOME_AMD_H
#define GENOME_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    GK_OK = 0,
    GK_E_INVALID = -1,        /* bad argument (NULL handle, negative size, ...) */
    GK_E_KLEN = -2,           /* key length != the map's k  (ArrayDNAMap.scala:182,187,192,199,206) */
    GK_E_UNSUPPORTED_K = -3,  /* k outside 2..31, 34..64 */
    GK_E_CAPACITY = -4,       /* table could not grow / export buffer too small */
    GK_E_HIP = -5,            /* HIP runtime error (message has the hipError string) */
    GK_E_NODEVICE = -6,       /* no usable gfx950 device */
    GK_E_FORMAT = -7,         /* malformed `.bin` read stream or FASTQ text, or a malformed / corrupt graph file (gk_graph_load) */
    GK_E_STATE = -8,          /* operation not valid in the handle's current state */
    GK_E_COMM = -9            /* RCCL missing or a collective failed (message has the RCCL error string) */
} gk_status;

typedef struct gk_ctx gk_ctx;       /* one device + stream; replaces ActorsHome.system (S/scripts/ActorsHome.scala:20-30) */
typedef struct gk_map gk_map;       /* one ArrayDNAMap[Int] partition, resident in HBM */
typedef struct gk_graph gk_graph;   /* a MapGraph, resident in HBM */
typedef struct gk_prefilter gk_prefilter;   /* exact two-pass singleton pre-filter (2-bit counters) */
typedef struct gk_dist gk_dist;     /* one rank of a PartitionedDNAMap spread over the GPUs of a node (RCCL communicator) */
typedef struct gk_fastq gk_fastq;   /* a FASTQ -> `.bin` conversion in progress (Convert2bin, S/scripts/Convert2bin.scala) */

/* ---- context ---------------------------------------------------------------------------- */
int gk_device_count(void);                       /* number of HIP devices, 0 if none / no runtime */
int gk_ctx_create(int device, gk_ctx **out);
void gk_ctx_destroy(gk_ctx *ctx);
const char *gk_last_error(const gk_ctx *ctx);    /* ctx may be NULL: last error of the calling thread */
int gk_ctx_device(const gk_ctx *ctx);
int gk_ctx_sync(gk_ctx *ctx);                    /* hipStreamSynchronize on the context stream */
/* Device buffers of 1 MiB and more that the library frees (tables, key scratch, graph arrays, gk_dev_free) are parked in the
 * context — up to a third of the device's memory — and handed out again by size: hipMalloc / hipFree of multi-GB blocks cost
 * milliseconds to seconds, and freshly freed memory is scrubbed on the copy engines while the next upload wants them.
 * gk_ctx_trim gives everything parked back to the device (gk_map_trim does so too); gk_ctx_destroy always does. */
int gk_ctx_trim(gk_ctx *ctx);
/* Device memory this context holds in blocks of 1 MiB and more (tables, key scratch, graph arrays, gk_dev_alloc): *live = bytes
 * handed out now, *peak = their high-water mark since the last reset, *parked = bytes waiting in the block pool; any may be
 * NULL.  reset_peak != 0 restarts the high-water mark at the current value.  (What DESIGN.md's bytes-per-key tables are
 * checked against; the reference's counterpart is the JVM heap it logs, -Xmx in project/Build.scala:44.) */
int gk_ctx_mem_stats(gk_ctx *ctx, uint64_t *live, uint64_t *peak, uint64_t *parked, int reset_peak);
/* Plan as if the device had `bytes` of memory (0 = all of it, the default): the sizing decisions that look at free memory — the
 * load factor of the table the graph phase reads, the key scratch of an insert batch — then use min(free, bytes - live).  For a
 * GPU shared with other work, and for rehearsing an 8-GPU replica's budget at an eighth of its size. */
int gk_ctx_set_mem_budget(gk_ctx *ctx, uint64_t bytes);
/* Pinned host memory: gk_map_count_reads / gk_prefilter_add_reads read the caller's `.bin` buffer with asynchronous copies
 * that overlap the insert kernels only if the buffer is page-locked — allocate it here, or register an existing one (a JNI
 * direct ByteBuffer's address) for as long as it is passed in.  Pageable buffers work, at a staged copy's speed. */
int gk_host_alloc(gk_ctx *ctx, size_t nbytes, void **host_ptr);
int gk_host_free(gk_ctx *ctx, void *host_ptr);
int gk_host_register(gk_ctx *ctx, void *host_ptr, size_t nbytes);
int gk_host_unregister(gk_ctx *ctx, void *host_ptr);
/* raw device memory helpers for callers without their own allocator (tests, the C++ host side) */
int gk_dev_alloc(gk_ctx *ctx, size_t nbytes, void **dev_ptr);
int gk_dev_free(gk_ctx *ctx, void *dev_ptr);
int gk_dev_upload(gk_ctx *ctx, void *dev_dst, const void *host_src, size_t nbytes);
int gk_dev_download(gk_ctx *ctx, void *host_dst, const void *dev_src, size_t nbytes);
/* What this card streams, measured: gbps3 = {copy (bytes read + written), fill (written), sum (read)} in GB/s over two
 * scratch buffers of nbytes each, `reps` launches of each kernel.  The yardstick SURVEY.md §8(d) asks for beside the nominal
 * HBM peak (bench.py reports the pipeline's traffic rate against it); no reference counterpart. */
int gk_dev_stream_bench(gk_ctx *ctx, size_t nbytes, int reps, double *gbps3);

/* ---- DNAMap[Int]: trait at S/ds/ArrayDNAMap.scala:49-60 ----------------------------------- */
/* new ArrayDNAMap[Int](k)  (ArrayDNAMap.scala:62-72).  capacity_hint = expected number of distinct
 * keys (0 = default); the table is pre-sized from it and grows by rehashing when a batch could
 * push the load factor past 0.75 (the reference's 0.3/0.7 rescale, :217-230, is unobservable). */
int gk_map_create(gk_ctx *ctx, int k, uint64_t capacity_hint, gk_map **out);
/* The same for a map that is FILLED ONCE with `keys` keys (a merge of partitions, a load from a file) and then read by
 * gk_graph_build: its table is sized the way the graph phase wants it — as sparse as memory allows, load 0.25 down to 0.7
 *  — which is also how gk_dist_gather_map sizes the table it returns and gk_map_filter_lt the one it leaves. */
int gk_map_create_for_graph(gk_ctx *ctx, int k, uint64_t keys, gk_map **out);
void gk_map_destroy(gk_map *m);
int gk_map_k(const gk_map *m);
int gk_map_clear(gk_map *m);                               /* back to an empty table of the same capacity */
/* How batches are inserted.  0 = auto (cost model), 1 = direct: one global CAS/add per k-mer
 * (k_count_reads / k_add_keys), 2 = partitioned: radix-partition the batch by 64-KiB table segment
 * and build each segment in LDS (gk_partition.hip).  Results are identical; only speed differs. */
int gk_map_set_insert_path(gk_map *m, int path);
int gk_map_size(gk_map *m, uint64_t *n);                   /* DNAMap.size :50 (live keys) */
int gk_map_slots(gk_map *m, uint64_t *slots);              /* current table capacity in slots */
/* Invariants of the table, checked on the device (the reference prints `nodeMap.size` next to the expected total,
 * Graph.scala:117): *live = live slots (== gk_map_size), *bad_slots = keys that are stored twice or in a segment
 * their hash does not name (must be 0), *sum_counts = sum of all counts (== occurrences inserted), *checksum = an
 * order-independent 64-bit checksum of the (key, count) set: two maps hold the same table iff (live, sum, checksum)
 * agree — whatever their sizes, slot orders and insert histories (partitions of one table ADD UP: the checksum of a
 * PartitionedDNAMap is the sum of its partitions' checksums mod 2^64).  Any may be NULL.
 * The checksum, exactly (tests/checksum_ref.py restates it; 64-bit arithmetic mod 2^64 throughout).  mix64(x): x ^= x >> 33;
 * x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33.  G = 0x9e3779b97f4a7c15.  With (lo, hi) the key
 * as it crosses this ABI:
 *     checksum = sum over the live entries of mix64(kh + count * G),
 *     kh = mix64(lo ^ 0x243f6a8885a308d3)                       for k <= 31,
 *     kh = mix64(lo ^ mix64(hi ^ 0x13198a2e03707344))           for k >= 34. */
int gk_map_verify(gk_map *m, uint64_t *live, uint64_t *bad_slots, uint64_t *sum_counts, uint64_t *checksum);
/* The count spectrum of the table: how many distinct k-mers occur exactly c times (what any k-mer counter reports: the coverage
 * peak, the error valley, a genome-size estimate).  One streaming pass over the slots on the device; nothing but the histogram
 * crosses to the host.  No reference counterpart: GraphBuilder.scala:30 hardcodes the cutoff this exists to choose.
 *   hist[0] = 0;  hist[c] = live keys with count exactly c, 1 <= c <= bins-2;  hist[bins-1] = live keys with count >= bins-1 (the
 *   overflow bin).  `hist` holds `bins` entries, 2 <= bins <= 1<<20 (GK_E_INVALID otherwise, and for a NULL hist).
 *   *distinct (== gk_map_size), *occurrences (== gk_map_verify's sum_counts) and *max_count (the largest count; 0 for an empty
 *   map) are exact whatever `bins` is; any of the three may be NULL.
 * The table is not changed.  A new or cleared map gives all zeros without its slots being read. */
int gk_map_spectrum(gk_map *m, uint64_t *hist, uint32_t bins, uint64_t *distinct, uint64_t *occurrences, uint32_t *max_count);
/* The deleteAll cutoff a spectrum suggests.  Pure host code: no context, runs without a GPU.  Only c in [min_count, bins-2] is
 * looked at, never the overflow bin:
 *   1. r = the smallest c in the range with hist[c] < hist[c+1] (c+1 <= bins-2).  None: GK_OK with *valley = *peak = 0 and
 *      *genome_size = 0 — "no valley" (callers then fall back to the reference's 3 and say so).
 *   2. *peak = the c > r with the largest hist[c]; on a tie the smallest c.
 *   3. *valley = the c in [min_count, *peak] with the smallest hist[c]; on a tie the smallest c.
 *   4. *genome_size = floor(sum over c = *valley .. bins-2 of c * hist[c] / *peak).
 * Use rounds = *valley: gk_map_filter_lt(*valley) keeps the counts >= *valley.  min_count is 1 normally, and 2 for a table counted
 * through the singleton pre-filter (gk_map_count_reads_prefiltered), whose bin 1 is incomplete by construction; 0 is
 * GK_E_INVALID, as are a NULL hist and bins outside 2 .. 1<<20.  Any out-pointer may be NULL. */
int gk_spectrum_cutoff(const uint64_t *hist, uint32_t bins, uint32_t min_count, uint32_t *valley, uint32_t *peak, uint64_t *genome_size);
/* Upper bound on the k-mer windows one partitioned insert batch holds when a call brings more windows than the
 * table has room for (the batch's key scratch is ~17 x W bytes per window); 0 = default (64 GiB of keys per buffer or as much scratch as the table itself holds, half of the free HBM at most). */
int gk_map_set_max_batch_keys(gk_map *m, uint64_t keys);
/* Release the scratch the handle keeps between calls (key buffers of the partitioned insert, staging of host streams,
 * point-query scratch).  The table is untouched; the next call allocates what it needs again. */
int gk_map_trim(gk_map *m);

/* FreqFilter.add over a stream of reads (S/data/FreqFilter.scala:28-36, 44-48):
 * for every read with len >= k, every window in order -> reverse complement -> orientation with
 * the smaller signed hashCode (tie: reverse complement) -> update(y, 1, _+1).
 * `bin` is the reference `.bin` record stream [len:u8][ceil(len/4) bytes] x nreads
 * (S/data/PairedEndData.scala:20-36); *occurrences (may be NULL) = number of windows counted.
 * The table grows as needed.  A call whose windows exceed the table's room is not assumed to bring that many NEW
 * keys (sequencing coverage: mostly repeats): the insert pipeline samples the distinct keys it sees and sizes the
 * table for those (gk_map_stats: "est_new_distinct_last_batch"). */
int gk_map_count_reads(gk_map *m, const uint8_t *bin_host, size_t nbytes, uint64_t nreads, uint64_t *occurrences);
/* Start uploading the head of a `.bin` stream NOW (asynchronously, on the copy stream, into the staging area the map is not
 * using) and return: the next gk_map_count_reads on THIS map whose stream starts at the same address then finds its first chunk
 * on the device and scatters it in one launch.  A streaming caller prefetches batch i+1 before it counts batch i: the upload
 * runs beside batch i's fine level.  (gk_map_count_reads does the same by itself between the chunks of ONE long stream.)  The
 * buffer must be page-locked (gk_host_alloc / gk_host_register) for the copy to be asynchronous, and must stay unchanged until
 * the count that consumes it has returned.  Reference: the reader thread of S/data/FreqFilter.scala:44-51 running ahead of
 * the inserts through the actors' mailboxes. */
int gk_map_prefetch_reads(gk_map *m, const uint8_t *bin_host, size_t nbytes, uint64_t nreads);
/* same, records already in HBM at a fixed stride 1+ceil(read_len/4); read_len = the LONGEST record (shorter ones
 * are fine).  Device records are untrusted input: a length byte above read_len is clamped, never followed, and
 * the call then fails with GK_E_FORMAT (the map's contents are unspecified: clear it). */
int gk_map_count_reads_dev(gk_map *m, const void *dev_records, uint64_t nreads, int read_len, uint64_t *occurrences);

/* ---- spectral read correction: this project's own rule (the reference has none: GraphBuilder.scala:30 hardcodes rounds = 3 and
 * lives with the k true k-mers that every wrong base costs) ----
 * Inputs: `counts`, a k-mer table of some k (either slot layout, filtered or not); a threshold solid >= 1; a `.bin` record stream.
 * The COUNT of a window is what gk_graph_edge_coverage defines: the entry of its hash-rule orientation, 0 if there is none; the two
 * stored orientations add up on a hash tie and in a table that took verbatim keys; a palindrome is one key.  A window is SOLID iff
 * its count >= solid, else WEAK.
 * For each record of L bases let n = L - k + 1.  n <= 0: the record is copied unchanged and counted as short.  Otherwise
 * s[0..n-1] are the solid flags of the windows of the INPUT record, and a weak run is a maximal [a, b] with s = 0.  Each weak run
 * is judged on its own, from the input record only.  With m = b - a + 1:
 *   1. Shape.  whole read (a = 0 and b = n-1): skipped;  head run (a = 0, b < n-1): needs m <= k, then p = b;  tail run (a > 0,
 *      b = n-1): needs m <= k, then p = a + k - 1;  interior run (a > 0, b < n-1): needs m = k, then p = b;  anything else is
 *      skipped.  In every accepted case the windows that contain base p are exactly [a, b].
 *   2. Candidates.  Each of the three bases c != read[p] is valid iff every window of [a, b] is solid once read[p] := c.
 *   3. Decision.  Exactly one valid c: base p becomes c (corrected).  Two or three: ambiguous, nothing changes.  None: unresolved,
 *      nothing changes.
 * So: runs never share a window and a correction touches only its own run's windows — the result depends neither on order nor
 * on scheduling; every window of a corrected run is solid in the output and all other windows are unchanged; correcting the
 * output again with the same map and `solid` changes nothing; the output has the framing of the input byte for byte (the same
 * length bytes, the same byte count, the padding bits of a record's last byte copied as they are): only the 2-bit fields of
 * corrected bases differ.  The map is never changed.  A new or cleared map is an empty table: every window is weak, nothing is
 * corrected, and its slots are not read.
 * stats (may be NULL) receives GK_CORRECT_NSTATS values, indexed by the names below; runs = corrected + ambiguous + unresolved +
 * skipped, always.
 * Host form: ragged streams are fine; the framing is validated on the host first, as gk_map_count_reads validates it
 * (GK_E_FORMAT, nothing written); the stream goes through the device in chunks; bin_out holds nbytes and may be bin_host.
 * Device form: fixed stride 1 + ceil(read_len / 4), shorter records inside the stride are fine; dev_out may be dev_records itself
 * (in place), any other overlap is GK_E_INVALID; a length byte above read_len is clamped, never followed, and the call then
 * fails with GK_E_FORMAT (the output is unspecified).
 * GK_E_INVALID: solid = 0, a NULL handle, NULL buffers with nreads > 0. */
enum {
    GK_CORRECT_READS = 0,      /* records */
    GK_CORRECT_SHORT = 1,      /* records shorter than k */
    GK_CORRECT_WINDOWS = 2,    /* windows */
    GK_CORRECT_WEAK = 3,       /* weak windows of the input */
    GK_CORRECT_RUNS = 4,       /* weak runs */
    GK_CORRECT_CORRECTED = 5,  /* runs with exactly one valid replacement: bases changed */
    GK_CORRECT_AMBIGUOUS = 6,  /* runs with two or three */
    GK_CORRECT_UNRESOLVED = 7, /* runs with none */
    GK_CORRECT_SKIPPED = 8,    /* runs skipped for their shape */
    GK_CORRECT_CHANGED = 9,    /* records with at least one base changed */
    GK_CORRECT_NSTATS = 10
};
int gk_reads_correct(gk_map *counts, const uint8_t *bin_host, size_t nbytes, uint64_t nreads, uint32_t solid,
                     uint8_t *bin_out, uint64_t *stats);
int gk_reads_correct_dev(gk_map *counts, const void *dev_records, uint64_t nreads, int read_len, uint32_t solid,
                         void *dev_out, uint64_t *stats);

/* DNAMap.update(key, 1, _+1) for a batch of keys taken verbatim (no canonicalisation):
 * PartitionedDNAMap's owner-side insert (Messages.update1, ArrayDNAMap.scala:39).  Keys are
 * W = 1 (k<=32) or 2 (k>32) uint64 each.  The map notices when a verbatim key is not the hash-rule orientation of
 * its k-mer (FreqFilter.scala:31-32): gk_graph_build then probes both strands for every `contains`, exactly as
 * Graph.scala:270 does, instead of the one probe a canonically filled table needs. */
int gk_map_update_inc(gk_map *m, const uint64_t *lo, const uint64_t *hi, uint64_t n);
/* device keys, interleaved W words per key ([lo] or [lo,hi]) as gk_shard_reads_dev emits them */
int gk_map_update_inc_dev(gk_map *m, const void *dev_keys, uint64_t n);
/* update(key, v0=c, f=_+c): adds counts of pre-aggregated keys (merging exported partitions) */
int gk_map_add_counts(gk_map *m, const uint64_t *lo, const uint64_t *hi, const int32_t *counts, uint64_t n);

/* update(key, c, _ + c) for every (key, c) of `src` (same context, same k), device to device in bounded chunks: merges the
 * partitions of a PartitionedDNAMap that share a device (the one-device counterpart of gk_dist_gather_map).  `src` is unchanged. */
int gk_map_add_map(gk_map *dst, gk_map *src);

/* DNAMap.deleteAll((k, v) => v < rounds)  (FreqFilter.scala:55; ArrayDNAMap.scala:164-173, 212-215) */
int gk_map_filter_lt(gk_map *m, int32_t rounds);

/* DNAMap.apply / contains for a batch (ArrayDNAMap.scala:90-101, 232): counts_out[i] = value or
 * -1 when absent; found_out[i] = 0/1.  Either output may be NULL.  One strand only, as the trait. */
int gk_map_get_batch(gk_map *m, const uint64_t *lo, const uint64_t *hi, uint64_t n, int32_t *counts_out, uint8_t *found_out);

/* Container.iterator / mapReduce(identity) (ArrayDNAMap.scala:175-178, 234-241): every live
 * (key, count) in ascending slot index.  Which slot a key sits in is the table's business (its geometry, its insert
 * history), so callers sort for comparison; what the order does promise is that two exports of an unchanged table agree and
 * that keys come out segment by segment and, inside a segment, slot by slot: a probe chain in chain order, except that the
 * part of it that wrapped past the segment's end comes first (tests/test_adversarial_keys_gpu.py reads positions off this).
 * If cap < live count the call fails with GK_E_CAPACITY and *n holds the required size. */
int gk_map_export(gk_map *m, uint64_t *lo, uint64_t *hi, int32_t *counts, uint64_t cap, uint64_t *n);

/* JSON counters: capacity, size, occurrences, grows, last kernel time ... (SURVEY.md §5 metrics), and which member of each
 * kernel family the map's LAST partitioned batch launched (noted on the host where the choice is made; "none" / 0 before the first):
 * "last_p2" ("plain" | "sorted" | "wide" | "wide_sorted": the L1 scatter of fixed-stride records; "exact": ragged records, behind
 * a histogram pass; "keys" | "keys_exact": key arrays), "last_fine" ("exact" | "overprovisioned"), "last_p4" ("sort4096" |
 * "sort8192" | "sort12288" | "sort6144" | "direct": keys per LDS sort of the fine scatter), "last_p4_stripes", "last_p4_pieces",
 * "last_nb1", "last_nb2" (integers: stripes and pieces of that batch, the table's L1 buckets and fine buckets per L1 bucket),
 * "last_slot" ("count12" | "slot16" | "slot24": the slot type the segments were built in), and "last_filter" ("streaming"
 * | "classic": the form the last gk_map_filter_lt took).  A batch that was abandoned for the direct path ("retries_direct") still leaves the names of what it had launched.  2 KiB holds the text. */
int gk_map_stats(gk_map *m, char *json, size_t cap);
/* duration (ms, HIP events on the context stream) and occurrence count of the most recent
 * insert+count kernel launched by gk_map_count_reads[_dev] — used by bench.py's roofline. */
int gk_map_last_count_kernel(gk_map *m, float *ms, uint64_t *occurrences);
/* per-phase device time (ms, HIP events) of the most recent insert: ms5 = {hist1, scatter1, hist2,
 * scatter2, seg_insert} for the partitioned path; {kernel, 0, 0, 0, 0} for the direct path. */
int gk_map_last_phase_ms(gk_map *m, float *ms5);

/* ---- PartitionedDNAMap: owner routing (S/ds/PartitionedDNAMap.scala:60-63) ----------------- */
/* Extract + canonicalise every k-mer of fixed-length device reads and bucket the canonical keys
 * by owner partition.  The owner is a strand-symmetric minimizer hash mod P (not `hashCode mod P`:
 * the partition function is unobservable in results), so both orientations of a
 * k-mer — and both candidates of the hash-rule tie — land on the same partition.
 * dev_keys_out receives the keys grouped by owner (W uint64 per key), capacity keys_cap keys;
 * counts_host[p] = number of keys for owner p (sum = occurrences).  Exchange the groups
 * (RCCL all-to-all) and feed what a rank receives to gk_map_update_inc_dev. */
int gk_shard_reads_dev(gk_ctx *ctx, int k, const void *dev_records, uint64_t nreads, int read_len, int P,
                       void *dev_keys_out, uint64_t keys_cap, uint64_t *counts_host);
/* The same routing, shipped as SUPER-K-MERS: every maximal run of consecutive same-owner windows of
 * a read becomes one record — the run's bases in the `.bin` framing [len:u8][2-bit bases] inside a
 * fixed slot of gk_skm_slot_bytes(k) bytes (16 for k<=31, 32 for k>=34; longer runs are split).
 * ~8x fewer bytes than 8/16-B keys cross xGMI; the owner re-extracts and canonicalises, exactly as
 * FreqFilter.add does on the original reads: feed what a rank receives to
 * gk_map_count_superkmers_dev.  dev_out is cut into P regions of out_cap_records / P slots; owner p's
 * records fill the start of region p; rec_counts_host[p] / kmer_counts_host[p] = records / windows
 * for owner p.  If a region is too small the call fails with GK_E_CAPACITY after filling the counts
 * (max of rec_counts_host = slots a region needs); retry with a larger buffer.  A region that holds
 * exactly its records is large enough; slots of a region past its records are not written.
 * A read's length byte may be below read_len (a shorter read in the same stride; the bytes past
 * its last base are ignored); a read shorter than k has no window and gives no record.
 * What a receiver may rely on: every window of every read appears in exactly one record; every
 * window of a record is at its owner (gk_owner_of); k <= len <= (slot - 1) * 4 for the length byte
 * of every record; the slot's bits past the last base are zero.
 * How the runs are cut is THIS VERSION's rule, pinned by tests/route_ref.py and
 * tests/test_route_gpu.py, and nothing a receiver may build on: a read of `len` bases has
 * len - k + 1 windows; they are taken in blocks of 64 counted from the read's first window; inside
 * a block every maximal run of equal owners is cut, from its start, into pieces of at most
 * rmax = (slot - 1) * 4 - k + 1 windows; a piece of wl windows starting at window p is one record:
 * byte 0 = wl + k - 1, then bases p .. p + wl + k - 2 of the read.  The ORDER of the records inside
 * a region is unspecified (it differs from call to call). */
int gk_skm_slot_bytes(int k);
int gk_shard_superkmers_dev(gk_ctx *ctx, int k, const void *dev_records, uint64_t nreads, int read_len, int P,
                            void *dev_out, uint64_t out_cap_records, uint64_t *rec_counts_host, uint64_t *kmer_counts_host);
int gk_map_count_superkmers_dev(gk_map *m, const void *dev_records, uint64_t nrecords, uint64_t kmers_total, uint64_t *occurrences);
/* owner of one key under the same function (host-side, for tests and for routing point queries) */
int gk_owner_of(int k, uint64_t lo, uint64_t hi, int P);
/* *foreign = live keys of partition p's table whose owner (of P) is not p — 0 for a correctly routed PartitionedDNAMap */
int gk_map_count_foreign(gk_map *m, int P, int p, uint64_t *foreign);

/* ---- DNAMap[T] with values and multimap inserts: the rest of the trait (S/ds/ArrayDNAMap.scala:49-60) -------------- */
/* A second kind of map, for T = a 64-bit value (GraphPosition, Long): putNew stores a key as often as it is put, getAll
 * returns every value stored under a key, update(key, v) inserts or overwrites, apply returns the first value in probe order.
 * Same HBM table layout as gk_map; nothing is deleted from these maps.  Used by gk_graph_position_map (Graph.getGraphMap). */
typedef struct gk_vmap gk_vmap;
int gk_vmap_create(gk_ctx *ctx, int k, uint64_t capacity_hint, gk_vmap **out);     /* new PartitionedDNAMap[GraphPosition](k), Graph.scala:92 */
void gk_vmap_destroy(gk_vmap *m);
int gk_vmap_k(const gk_vmap *m);
int gk_vmap_size(gk_vmap *m, uint64_t *n);                                         /* DNAMap.size :50 — entries, duplicates included */
/* DNAMap.putNew(key, v) (:55; Container.putNew ArrayDNAMap.scala:152-162), batched: no duplicate check — a multimap.
 * BOUND (the reference has none): all copies of a key live in the one 32 KiB / 24 KiB segment its hash names, so one key can be
 * stored at most 2048 times (k <= 31), 1024 times (34 <= k <= 63) or 256 times (k = 64), less what else shares the segment;
 * beyond that the call fails with GK_E_CAPACITY, the batch's other entries stay stored (a failed batch is NOT rolled back;
 * gk_vmap_size tells what is in).  Graph.getGraphMap stores a k-mer once per graph position: far from the bound. */
int gk_vmap_put_new_batch(gk_vmap *m, const uint64_t *lo, const uint64_t *hi, const uint64_t *values, uint64_t n);
/* DNAMap.update(key, v) (:53; Container.update :115-127), batched: insert, or overwrite the first entry of the key; for a key
 * that occurs several times in one batch the LAST occurrence wins, as in the reference's sequential loop */
int gk_vmap_update_batch(gk_vmap *m, const uint64_t *lo, const uint64_t *hi, const uint64_t *values, uint64_t n);
/* DNAMap.getAll(key) (:52; Container.getAll :103-113), batched, CSR output: the values of key i are
 * values_out[offsets_out[i] .. offsets_out[i+1]) (offsets_out has n + 1 entries); *total = offsets_out[n].  If values_cap <
 * *total the offsets are still filled and the call fails with GK_E_CAPACITY.  Order inside a key's run: most recently probed
 * first, as the reference's list — callers treat it as a set (GraphSimplifier.scala:192-217). */
int gk_vmap_get_all_batch(gk_vmap *m, const uint64_t *lo, const uint64_t *hi, uint64_t n, uint64_t *offsets_out, uint64_t *values_out,
                          uint64_t values_cap, uint64_t *total);
/* DNAMap.apply(key) (:51), batched: first value in probe order; found_out[i] = 0/1 (may be NULL) */
int gk_vmap_get_batch(gk_vmap *m, const uint64_t *lo, const uint64_t *hi, uint64_t n, uint64_t *values_out, uint8_t *found_out);
/* Container.iterator: every (key, value), unspecified order */
int gk_vmap_export(gk_vmap *m, uint64_t *lo, uint64_t *hi, uint64_t *values, uint64_t cap, uint64_t *n);

/* GraphPosition (S/data/graph/GraphPosition.scala) as a 64-bit value: NodeGraphPosition(id) = id;
 * EdgeGraphPosition(id, dist) = 1<<63 | id<<32 | dist.  Ids are this library's node / edge ids (gk_graph_*_by_id). */
#define GK_POS_IS_EDGE(v) (((v) >> 63) != 0)
#define GK_POS_ID(v) ((uint32_t)(GK_POS_IS_EDGE(v) ? (((v) >> 32) & 0x7fffffffu) : ((v) & 0xffffffffu)))
#define GK_POS_DIST(v) ((uint32_t)((v) & 0xffffffffu))

/* ---- PartitionedDNAMap over N GPUs: one rank (process) per GPU, RCCL over xGMI ---------------- */
/* Reference: `new PartitionedDNAMap[Int](k)` deploys one ArrayDNAMap actor per storage node and sends one message per k-mer
 * occurrence to its owner (S/ds/PartitionedDNAMap.scala:20-47).  Here every rank holds ONE partition (a gk_map it created on
 * its own context), routes the k-mers of ITS reads as super-k-mer records and exchanges them with one all-to-all per call.
 * Bootstrap: rank 0 calls gk_dist_unique_id and hands the 128 bytes to the other ranks by any means the host has (the JVM
 * driver's own channel, a file, MPI, torch.distributed in bench.py); every rank then calls gk_dist_create — collectively.
 * RCCL is loaded on first use (dlopen); without it these calls fail with GK_E_COMM and nothing else is affected.
 * All gk_dist_* calls that move data are COLLECTIVE: every rank of the communicator must make them, in the same order. */
int gk_dist_unique_id(void *id128);                                   /* out: 128 bytes */
int gk_dist_create(gk_ctx *ctx, int rank, int world, const void *id128, gk_dist **out);
void gk_dist_destroy(gk_dist *d);
int gk_dist_rank(const gk_dist *d);
int gk_dist_world(const gk_dist *d);
int gk_dist_barrier(gk_dist *d);
/* all-reduce of up to 32 doubles in place (op_max: 0 = sum, 1 = max) — for the host's own bookkeeping (timings, totals) */
int gk_dist_allreduce_f64(gk_dist *d, double *values, int n, int op_max);
/* FreqFilter.add over THIS rank's reads, every k-mer counted by its owner rank (PartitionedDNAMap.update, :41-43):
 * route (gk_shard_superkmers_dev, P = world) -> exchange counts -> exchange records -> gk_map_count_superkmers_dev on `local`.
 * *occurrences_sent = windows of this rank's reads, *occurrences_owned = windows this rank counted (sums over ranks agree). */
int gk_dist_count_reads_dev(gk_dist *d, gk_map *local, const void *dev_records, uint64_t nreads, int read_len,
                            uint64_t *occurrences_sent, uint64_t *occurrences_owned);
/* FreqFilter.add over THIS rank's share of the reads as a HOST `.bin` stream ([len:u8][ceil(len/4) bytes] per record, lengths
 * 0..255 and ragged — what Convert2bin writes), every k-mer counted by its owner rank.  Ranks may pass streams of any length,
 * nreads == 0 included.  The stream is cut into chunks by gk_map_count_reads' rules (bounded staging; a run of equal-length
 * records takes the fixed-stride route, a ragged chunk an offset-framed one) and streamed through route_begin / count_routed
 * three batches deep, with the upload of the next chunks on the context's second stream.  Every rank walks its whole stream's
 * framing before anything is exchanged: a truncated or malformed stream on ANY rank returns GK_E_FORMAT on EVERY rank, nothing
 * moves and every `local` is unchanged.  A rank with fewer chunks routes empty batches, so that every rank issues the same
 * operations.  A failure after streaming began (an exchange dropped, a HIP error on one rank) returns an error on every rank and
 * leaves nobody waiting; `local` then holds an UNSPECIFIED subset of the counts and must be cleared (gk_map_clear) before
 * reuse.  Needs no routes begun with gk_dist_route_begin outstanding (GK_E_STATE on this rank, GK_E_COMM on the others).  The
 * staging areas (one per batch in flight) stay on the handle until gk_dist_destroy and count in gk_ctx_mem_stats.
 * *occurrences_sent = windows of this rank's stream, *occurrences_owned = windows this rank counted (sums over ranks agree). */
int gk_dist_count_reads(gk_dist *d, gk_map *local, const uint8_t *bin_host, size_t nbytes, uint64_t nreads,
                        uint64_t *occurrences_sent, uint64_t *occurrences_owned);
/* The same in two halves, for a streaming loop: gk_dist_route_begin launches the routing of a batch on the context's second
 * stream and returns at once; gk_dist_count_routed waits for it, exchanges and counts.  Calling route_begin for batch i+1
 * BEFORE count_routed for batch i overlaps the routing kernel with the owner pipeline; with route_begin for batch i+2 before
 * it as well, count_routed(i) first posts the exchange of batch i+1 on the handle's own communication stream, so that those
 * records travel over xGMI while batch i is counted (three send buffers, two receive buffers; the rule depends only on the
 * number of begun batches, so every rank issues the same sequence of RCCL operations — all ranks must run the same loop).
 * The records of a begun batch must stay valid until its count_routed returns.  At most three batches may be begun and not
 * yet counted (GK_E_STATE otherwise; count_routed with none begun is GK_E_STATE too); they are counted first in, first out:
 * begin(0), begin(1), [begin(i+2), count_routed(i)]*, count_routed(last-1), count_routed(last).  A batch whose exchange
 * fails is dropped and the error returned by the count_routed whose turn it is.  A malformed record in a begun batch
 * (GK_E_FORMAT) may be reported by whichever count call on the context checks the flags next. */
int gk_dist_route_begin(gk_dist *d, int k, const void *dev_records, uint64_t nreads, int read_len);
int gk_dist_count_routed(gk_dist *d, gk_map *local, uint64_t *occurrences_sent, uint64_t *occurrences_owned);
/* wall ms of the last gk_dist_count_routed on this rank: {waiting for the route, exchange, owner count, total} */
int gk_dist_last_ms(gk_dist *d, float *ms4);
int gk_dist_size(gk_dist *d, gk_map *local, uint64_t *total);         /* PartitionedDNAMap.size (:31): sum over the partitions */
/* The spectrum of the WHOLE PartitionedDNAMap on every rank (gk_map_spectrum's outputs and rules; `bins` the same on every rank):
 * each rank takes the spectrum of its partition; the partitions are disjoint by owner, so the sum over the ranks of hist, distinct
 * and occurrences and the maximum of max_count are the whole map's.  COLLECTIVE: two all-reduces (uint64 max: largest count and a
 * status word; uint64 sum: the rest).  A rank whose local pass failed (a NULL `local` or one of another context included)
 * still takes part and says so in the status word: every rank then returns an error, nobody waits, and the handle stays usable.
 * That covers failures of the local pass only: a NULL `d` or `hist`, or bad `bins`, is GK_E_INVALID on the rank that passes it, before
 * the collective, like a wrong argument of any other gk_dist_* call (the other ranks would wait). */
int gk_dist_spectrum(gk_dist *d, gk_map *local, uint64_t *hist, uint32_t bins, uint64_t *distinct, uint64_t *occurrences, uint32_t *max_count);
/* deleteAll / filter_lt, stats, export are LOCAL: call gk_map_filter_lt etc. on `local` on every rank (:49-51 scatter, no data moves). */
/* The whole k-mer set on every rank, for Graph.buildGraph (the unitig walk crosses partitions arbitrarily):
 * all-gather of every partition's live (key, count), device to device and in bounded chunks (staging <= 0.7 GB to send, world x
 * that to receive), into a NEW map (*full, caller destroys it) sized the way the graph phase wants it.  A rank that fails
 * says so in the chunk's size word: every rank then returns an error for the same chunk and nobody waits in a receive. */
int gk_dist_gather_map(gk_dist *d, gk_map *local, gk_map **full);
/* The same gather with the classify of Graph.buildGraph done by the keys' OWNERS first (Graph.scala:320-329 shipped to every
 * partition, PartitionedDNAMap.scala:55-58; SURVEY.md section 8e "beyond counting"): every rank looks up the neighbours it owns
 * in its own partition and asks the other neighbours of their owners (per chunk: one all-to-all of canonical keys, one of answer
 * bytes), and each key's (incoming, outcoming) mask travels with it into *full.  gk_graph_build on *full then derives the
 * terminal k-mers from the masks in one streaming pass — the eight lookups per key are done once in the whole job instead of once
 * per rank.  The masks serve the FIRST gk_graph_build on *full; any change of its contents drops them (plain classify again).
 * Partitions that hold verbatim non-canonical keys on any rank: plain gather on every rank.  `local` is left in the graph
 * layout; its contents are unchanged.  Same failure behaviour as gk_dist_gather_map. */
int gk_dist_gather_classified_map(gk_dist *d, gk_map *local, gk_map **full);
/* neighbour lookups this rank has asked of other ranks in classified gathers since the handle was created */
int gk_dist_classify_queries(gk_dist *d, uint64_t *n);
/* The paired-end support over the ranks (GraphSimplifier.scala:172-186, 209-248: the driver sums the WalkingActors' counters
 * into one pathsMap).  Every rank holds a replica of the graph and has walked ITS share of the pairs into `sup`; afterwards
 * every rank's sup holds the sum over all ranks: every (e1, e2) count, bad pairs and walked orientations added up, the
 * distinct-pair count recomputed, keyed by THIS rank's edge ids.  The replicas need not number their edges alike: the pairs
 * travel in a canonical numbering (live edges ordered by (start k-mer, first base)), so the replicas must hold the same edges —
 * a fresh build or a retained one, before any node split (a split makes copies that share a start k-mer: GK_E_STATE).  Before
 * any payload moves the ranks agree on every rank's status and on equal content fingerprints of g; after the owners' merge
 * on "no count passed 2^32-1", and after the rebuild once more, before anything is swapped in.  If any of this fails on any
 * rank, every rank returns an error (GK_E_STATE for replicas that differ, GK_E_CAPACITY for an overflow), every sup is left
 * unchanged and no rank is left waiting in a receive.  Pairs go to an owner rank by a hash of the canonical (e1, e2): one
 * all-to-all of 12-byte records, the owners merge, then every owner's shard goes to every rank.  world <= 64 (gk_dist_create).
 * world == 1: only the checks run.  COLLECTIVE. */
typedef struct gk_support gk_support;
int gk_dist_reduce_support(gk_dist *d, gk_graph *g, gk_support *sup);

/* ---- Graph: S/data/graph/Graph.scala ------------------------------------------------------- */
/* Graph.buildGraph(k, kmersFreq) (:269-382): degree classification of every live key through
 * `contains` on both strands, one node per terminal k-mer (both strands), one edge per
 * (node, outgoing base) walked to the next terminal k-mer.  The map must hold the whole k-mer set
 * (merge partitions with gk_map_export + gk_map_add_counts first). */
int gk_graph_build(gk_map *m, gk_graph **out);
void gk_graph_destroy(gk_graph *g);
int gk_graph_counts(gk_graph *g, uint64_t *nodes, uint64_t *edges, uint64_t *total_edge_len); /* live */
/* CheckGraph.scala:37-41 over the live edges with length > longer_than (the reference: 200).  median = sorted[count/2], which is
 * what the reference logs as "N50"; n50 = the real one: lengths descending, the first length at which twice the running sum
 * reaches the total.  count == 0: everything 0.  Both strands' edges are counted, as in the reference.  One reduction and a radix
 * select by histogram passes on the device: the lengths are neither downloaded nor sorted. */
int gk_graph_contig_stats(gk_graph *g, uint64_t longer_than, uint64_t *count, uint64_t *sum, uint64_t *median, uint64_t *n50, uint64_t *max);
int gk_graph_simplify(gk_graph *g);          /* MapGraph.simplifyGraph :211-230 */
int gk_graph_remove_bubbles(gk_graph *g);    /* Graph.removeBubbles :125-149 */

/* ---- perfect cycles ---------------------------------------------------------------------------
 * The reference drops every circular sequence it assembles without a blemish (Graph.scala:375 "perfect cycles are ignored";
 * simplifyGraph :220-221 removes a node whose way in and way out are one edge), and so do gk_graph_build and gk_graph_simplify,
 * bit for bit.  The two entry points below keep them.  Nothing else changes: not the two plain calls, not the graph file.
 *
 * Cycle members.  An oriented k-mer u of the table is a member iff it has exactly one successor and one predecessor (so it is
 * not terminal by the classify's predicate, and not an isolated k-mer without neighbours either) and following successors from
 * u never reaches a terminal k-mer: what the plain build puts on no node and inside no edge.  Members form disjoint oriented
 * cycles under the successor map; the reverse complement of a cycle is a cycle, possibly the same one.
 * Anchors.  The anchor key of a k-mer x is min(x, rc x) as 2-bit-packed integers compared as (hi, lo): it depends on content
 * only, is the same for both strands, and does not depend on the table's orientation rule, slot order or capacity.  It is a
 * CONVENTION (any strand-symmetric total order would serve), not a measurement.  A member whose anchor key is its cycle's
 * minimum is an anchor.  Two different k-mers share a key only as x and rc x, so a cycle has one anchor — or two, when it is its
 * own reverse complement and its smallest k-mer is not a palindrome.
 * gk_graph_build_cycles = gk_graph_build, then: every anchor becomes a node with one out-edge, the arc from it to the next anchor
 * of its cycle (itself when it is the only one); seq = the bases appended on the way, len = the steps.  A cycle of L k-mers with
 * one anchor is a self-loop of len L whose path (L + k bases) ends in the anchor's k-mer again; a homopolymer is a self-loop of
 * one base.  Strand closure: rc maps a cycle onto a cycle and keeps keys, so the anchors of a cycle and of its reverse
 * complement are twins, and so are their arcs; in a self-complementary cycle with anchors x and rc x, rc maps the arc from x to
 * rc x onto a path from x to rc x, which successors being unique is the same arc: each of the two arcs is its own twin.
 * Ids: the plain build's nodes and edges keep theirs (a table without members gives the identical graph: ids, gk_graph_checksum,
 * gk_graph_id_fingerprint; with members, removing what was added leaves the plain build's graph).  Anchor nodes follow in pairs
 * — even id: the anchor that is its own key, odd id: its reverse complement (dead for a palindrome) — in table slot order;
 * the arcs follow the plain build's edges, one per anchor, in table slot order (stored orientation first).
 * stats6 = {cycle_kmers (oriented members), cycles (oriented), anchors (nodes added == edges added), self_complementary (cycles
 * equal to their reverse complement), longest (k-mers), rounds (doubling rounds of the minimum)}.  The summed len of the added
 * edges == cycle_kmers; anchors == cycles + cycles with two anchors.  No members: all 0, and nothing but one census pass ran.
 * GK_E_CAPACITY: 2^31 members or more.  stats6 may be NULL.
 *
 * gk_graph_simplify_keep_cycles = gk_graph_simplify, except: a node whose way in and way out are the same edge stays with it
 * (it is an anchor already), and in a cycle made only of merge-away nodes the nodes whose k-mer has the cycle's smallest anchor key
 * (one, or two twins) are kept, so that each arc between them is merged into one edge as any other chain.  Isolated nodes still go.
 * Where node copies (gk_graph_split_edges_by_spans, gk_graph_split_by_support) put the same k-mer on one such cycle more than
 * once, every node with the smallest key is kept: more than two anchors then, each arc still merged into one edge.
 * Idempotent.  On a graph with neither shape the result is gk_graph_simplify's, checksums and id fingerprint included.
 * stats4 = {kept_self_loops, cycles_merged (cycles of merge-away nodes that lost a node), anchors_kept, nodes_removed}; may be NULL.
 * Not there: a collective over ranks, circular references in the judge and the blocks, a `circular` tag in the FASTA records. */
int gk_graph_build_cycles(gk_map *m, gk_graph **out, uint64_t *stats6);
int gk_graph_simplify_keep_cycles(gk_graph *g, uint64_t *stats4);
/* MapGraph.removeEdge :191-195 for the edges leaving start[i] with first base base[i] */
int gk_graph_remove_edges(gk_graph *g, const uint64_t *start_lo, const uint64_t *start_hi, const uint8_t *base,
                          uint64_t n, uint64_t *removed);
/* Graph.components + retain(maxBy size) (:54-72, :161-165; GraphBuilder.scala:52-54); ties between
 * equal-size components go to the one holding the smallest k-mer. */
int gk_graph_retain_largest(gk_graph *g, uint64_t *kept_nodes, uint64_t *components);
/* GraphBuilder's two component histograms (GraphBuilder.scala:41-47) are group-bys of these two arrays: one entry per
 * connected component, nodes_per_component[i] = comp.size, edge_len_per_component[i] = sum of seq.size over the out-edges
 * of its nodes; order unspecified.  If cap < *n the call fails with GK_E_CAPACITY and *n holds the required size. */
int gk_graph_component_stats(gk_graph *g, uint32_t *nodes_per_component, uint64_t *edge_len_per_component, uint64_t cap, uint64_t *n);
/* Order-independent 64-bit checksums of the canonical serialisation: the node k-mer set, and the edge set
 * as (start k-mer, end k-mer, length, every base).  Two graphs with equal counts and checksums are the same graph.  The exact
 * formulas, and gk_graph_id_fingerprint's, stand with the graph file below, whose header stores all three. */
int gk_graph_checksum(gk_graph *g, uint64_t *nodes_checksum, uint64_t *edges_checksum);
/* How gk_graph_build spent its time: phase_ms6 = {degree classification (k_classify), terminals -> nodes + edge stubs,
 * unitig measurement (k_walk pass 0 or pointer jumping), pool reservation, unitig emission, node index + counts} (wall ms,
 * every phase ends in a stream sync); *walked_bases = bases emitted; *pointer_jumping = 1 if k_pj_* built the unitigs. */
int gk_graph_build_stats(gk_graph *g, float *phase_ms6, uint64_t *walked_bases, int *pointer_jumping);
/* When gk_graph_build ran on a minimizer-bucketed copy of the table (gk_ctx_set_option "graph_mbt" = 1): wall ms of building the
 * copy and its slots; 0 / 0 otherwise.  Diagnostics of an A/B switch. */
int gk_graph_bucketed_table_stats(gk_graph *g, float *build_ms, uint64_t *slots);
/* *flag = 1 when gk_graph_build took the degree masks that came with the table (gk_dist_gather_classified_map) instead of
 * running the neighbour lookups itself */
int gk_graph_classified_by_owners(gk_graph *g, int *flag);
/* Graph.getGraphMap (Graph.scala:90-119): putNew of every node's k-mer -> NodeGraphPosition(node id) and of the k-mers at
 * distance 1 .. len-1 along every edge -> EdgeGraphPosition(edge id, dist) into `vm` (same k, same context).  *entries =
 * number of entries added = sum of edge lengths + nodes - edges (the reference prints both side by side, :117; here the
 * equality is checked).
 * How many positions a k-mer has.  On a graph as gk_graph_build leaves it every k-mer lies on one node or at one distance of one
 * edge, so getAll gives one position or none, palindromes included: a k-mer that is its own reverse complement is either a node
 * (one node, which is its own twin) or the centre window of an edge that is its own twin (P(e) = its reverse complement), at
 * distance len / 2, once; it is not entered a second time for the other strand.  Two or more positions come from edits alone:
 * the node copies of gk_graph_split_by_support and the edge and node copies of gk_graph_split_edges_by_spans share their k-mers.
 * So the classes that need a list of two (`repeated` of gk_graph_thread_reads, `ambiguous` and `repetitive` of
 * gk_graph_pair_distances, `repetitive` of gk_graph_pair_links and of the placements) are empty on a fresh graph, whatever it
 * folds back on; and a pair whose two mates lie on one edge, a self-twin edge or a self-loop included, is `same_edge` for
 * gk_graph_pair_links: the table never holds a link (e, e). */
int gk_graph_position_map(gk_graph *g, gk_vmap *vm, uint64_t *entries);
/* Ids.  Node and edge ids are array indices (arbitrary, like the reference's AtomicLong ids; stable for a graph's lifetime).
 * gk_graph_node_lookup: the live node with this k-mer (smallest id if a node split left several) and, for base in 0..3, the id
 * of its out-edge whose sequence starts with that base; 0xffffffff = none. */
int gk_graph_node_lookup(gk_graph *g, uint64_t lo, uint64_t hi, int base, uint32_t *node_id, uint32_t *edge_id);
int gk_graph_nodes_by_id(gk_graph *g, const uint32_t *ids, uint64_t n, uint64_t *lo, uint64_t *hi, uint8_t *alive, uint32_t *in_deg, uint32_t *out_deg);
int gk_graph_edges_by_id(gk_graph *g, const uint32_t *ids, uint64_t n, uint32_t *start_node, uint32_t *end_node, uint64_t *len,
                         uint8_t *first_base, uint8_t *alive);
/* MapGraph.addNode(seq) (:172-176): a new node without edges (a node split creates nodes that share a sequence) */
int gk_graph_add_node(gk_graph *g, uint64_t lo, uint64_t hi, uint32_t *node_id);
/* MapGraph.replaceStart / replaceEnd (:197-209): re-attach one end of an edge to another node */
int gk_graph_replace_start(gk_graph *g, uint32_t edge_id, uint32_t new_start_node);
int gk_graph_replace_end(gk_graph *g, uint32_t edge_id, uint32_t new_end_node);
/* ids run from 0 to these bounds (dead nodes / edges keep theirs) */
int gk_graph_id_bounds(gk_graph *g, uint64_t *node_ids, uint64_t *edge_ids);
/* An id-exact fingerprint of the graph: a sum mod 2^64 over the live nodes (id, k-mer) and the live edges (id, start id, end id,
 * first base, length), each mixed through a 64-bit hash, plus the id bounds.  Two graphs share it iff (up to hash collisions)
 * their ids mean the same nodes and edges.  gk_graph_checksum is content-only and cannot tell that.  Note: two builds of one
 * table need not number alike (ids follow table slot order, output ranges come from atomic cursors). */
int gk_graph_id_fingerprint(gk_graph *g, uint64_t *fp);
/* MapGraph.removeEdge (:191-195) by edge id (each id once, as the reference's `toRemove` Set, GraphSimplifier.scala:270,316) */
int gk_graph_remove_edges_by_id(gk_graph *g, const uint32_t *edge_ids, uint64_t n, uint64_t *removed);

/* ---- edge coverage and tips: this project's own rules (the reference keeps no counts past buildGraph and removes no tips) ----
 * Coverage.  A live edge of `len` bases leaving the start node S has len + 1 k-mers: the windows of S ++ seq at distances
 * 0 .. len, both end nodes included — the strand-symmetric choice: an edge and its reverse-complement twin read the same numbers.
 * The count of a window is what `counts` holds for its hash-rule orientation (FreqFilter.scala:31-32), 0 if it holds none; where
 * the rule cannot tell the strands apart (equal hashes, the k-mer not its own reverse complement) and in a table that took
 * verbatim keys in either orientation, the counts of both stored orientations add up.  Per id asked for, in the order asked:
 * kmers[i] = len + 1, sum[i] = the sum of the counts, min_count[i] / max_count[i] over the same windows; a dead or out-of-range id
 * gives zeros.  *missing = the windows with no entry in `counts`, summed over the ids asked for (an id asked twice counts twice).
 * Any output pointer may be NULL.  `counts` may be any k-mer table of the graph's k on the graph's context, in either slot layout —
 * the table the graph was built from (the build leaves its counts alone), or one counted afresh for a loaded graph; a table of
 * another k or context, or a NULL handle: GK_E_INVALID.  Nothing is attached to the graph: the call is valid on a graph in any
 * state (merged edges, node copies), and neither the graph, its file format, checksum nor id fingerprint change. */
int gk_graph_edge_coverage(gk_graph *g, gk_map *counts, const uint32_t *edge_ids, uint64_t n, uint64_t *kmers, uint64_t *sum,
                           uint32_t *min_count, uint32_t *max_count, uint64_t *missing);
/* Tips.  One round, decided entirely from the graph's state at entry and then applied at once (the result depends neither on
 * scheduling nor on id order).  A live edge e (start u, end v, len bases, mean coverage sum_e / kmers_e as above) is removed iff
 *   len <= max_len, and a competitor f exists with STRICTLY higher mean coverage, and one of
 *   out-tip: v has out-degree 0 and in-degree 1, and u has out-degree >= 2; competitors are the other live out-edges of u;
 *   in-tip:  u has in-degree 0 and out-degree 1, and v has in-degree >= 2; competitors are the other live in-edges of v.
 * "e below f" is sum_e * kmers_f < sum_f * kmers_e, compared exactly as 128-bit integers; no floating point.  So: ties remove
 * nothing; an isolated short contig is kept; two tips at one junction beside a stronger third edge both go; the twin of an
 * out-tip is an in-tip with the same numbers, so a strand-closed edge set stays strand-closed.  Removal is MapGraph.removeEdge
 * (:191-195); nodes stay — the isolated dead ends and the junctions left with one way in and one way out are what the caller's
 * next simplifyGraph removes and merges.  *removed_edges = edges removed.  max_len == 0 removes nothing.  If any window of any
 * live edge is missing from `counts` the map is not this graph's: GK_E_STATE, and the graph is untouched.  Handles as above. */
int gk_graph_clip_tips(gk_graph *g, gk_map *counts, uint64_t max_len, uint64_t *removed_edges);
/* Distance.  dist[i] = min(Levenshtein(seq(e1[i]), seq(e2[i])), max_diff + 1): substitution, insertion and deletion cost 1
 * each, and seq is the edge's own bases, the ones after the start k-mer (gk_graph_export_edges' sequence).  Exact within the
 * band: an alignment of cost <= max_diff never leaves |i - j| <= max_diff, so nothing else is looked at; lengths that differ by
 * more than max_diff give max_diff + 1 without any comparison.  e1[i] == e2[i] (live) gives 0; a dead or out-of-range id on either
 * side gives 0xffffffff.  max_diff > 31: GK_E_INVALID (a band of 2 * max_diff + 1 <= 63 diagonals is one wave of the device).
 * n == 0 is GK_OK.  The graph is not changed.
 * Strand symmetry rests on this: two edges with the same start node share the prefix start.seq of their paths start.seq ++ seq,
 * two with the same end node the suffix end.seq; the Levenshtein distance does not change when a common prefix or suffix is
 * stripped, nor when both strings are reversed and complemented.  So for parallel edges the distance of the sequences IS the
 * distance of the paths, and the distance of their reverse-complement twins' sequences. */
int gk_graph_edge_distance(gk_graph *g, const uint32_t *e1, const uint32_t *e2, uint64_t n, uint32_t max_diff, uint32_t *dist);
/* Bubbles.  One round, decided entirely from the graph's state at entry and then applied at once, as the tips are.  Two live
 * edges are PARALLEL when they have the same start node and the same end node, by node id (the copies a node split leaves are
 * different nodes; the self-loops at one node are parallel to each other).  A live edge e is removed iff some other live edge f
 *   is parallel to e, and len_e <= max_len and len_f <= max_len, and distance(e, f) <= max_diff (as above), and
 *   e is STRICTLY below f in mean coverage: sum_e * kmers_f < sum_f * kmers_e, the 128-bit comparison of the tips over the same
 *   len + 1 windows.
 * So: ties remove nothing; the strongest edge of any group of similar parallel edges always survives; with e < f < g in coverage,
 * d(e,f) <= max_diff, d(f,g) <= max_diff and d(e,g) > max_diff, e and f both go; two edges that are each other's twins tie and
 * stay; the twins of a parallel pair are a parallel pair with the same coverages and the same distance, so a strand-closed edge
 * set stays strand-closed.  Removal is MapGraph.removeEdge (:191-195); nodes stay for the caller's next simplifyGraph.  max_len
 * == 0 removes nothing, and neither does max_diff == 0 (the out-edges of one node differ in their first base: their distance is
 * >= 1).  *removed_edges = edges removed.  *pairs_compared = the unordered pairs of live parallel edges within max_len whose
 * distance was computed: a pair whose lengths differ by more than max_diff does not count.  max_diff > 31: GK_E_INVALID.
 * Coverage is computed for the CANDIDATE edges only: those with a parallel edge, both within max_len.  If a window of a candidate
 * edge is missing from `counts` the map is not this graph's: GK_E_STATE, and the graph is untouched.  Handles as above.
 * gk_graph_remove_bubbles — the reference's rule: lengths within a fifth, no sequences, no coverage — is a different entry
 * point and unchanged. */
int gk_graph_pop_bubbles(gk_graph *g, gk_map *counts, uint64_t max_len, uint32_t max_diff, uint64_t *removed_edges, uint64_t *pairs_compared);
/* Weak connections.  One round, decided entirely from the graph's state at entry and then applied at once, as the tips and the
 * bubbles are (the result depends neither on scheduling nor on id order).  The tips remove dead ends and the bubbles the weaker of
 * two SIMILAR parallel edges; this removes an edge that is a proper connection by shape — both of its ends have another way on —
 * but is carried by a handful of reads where its neighbours are carried by many: a chimeric read, a coincidental overlap of errors,
 * a bubble arm too dissimilar for max_diff.  Coverage is gk_graph_edge_coverage's: len + 1 windows, both end nodes included, sum
 * and kmers per edge.  "R times e is below f" means sum_e * (R * kmers_f) < sum_f * kmers_e, compared exactly as 128-bit integers:
 * the tips' comparison with R * kmers_f in the place of kmers_f.  No floating point.  ratio > 65535: GK_E_INVALID — the bound
 * keeps R * kmers_f inside 64 bits for any edge that fits in memory (kmers < 2^48).
 * A live edge e (start u, end v, by node id) with len_e <= max_len is removed iff (A) or (B) holds:
 *   (A) connection, when ratio >= 1: u has out-degree >= 2, and v has in-degree >= 2, and some OTHER live out-edge f of u has
 *       `ratio` times e below f, and some OTHER live in-edge f' of v has `ratio` times e below f' (f' may be f);
 *   (B) floor, when floor >= 1: sum_e < floor * kmers_e (mean coverage strictly below `floor`), whatever the edge's shape.
 * ratio == 0 switches (A) off, floor == 0 switches (B) off, max_len == 0 removes nothing.  So:
 *   a tip is not a connection: an out-tip's v has in-degree 1, an in-tip's u out-degree 1 — (A) leaves both to gk_graph_clip_tips;
 *   ties remove nothing under (A), and with ratio = 1 the comparison is the tips' strict "below";
 *   under (A) the strongest out-edge of every node and the strongest in-edge of every node survive: an edge that is removed has a
 *   strictly stronger competitor at each end, and the maximum has none — (A) never takes a node's last way out or last way in;
 *   a self-loop at u competes with u's other out-edges and with u's other in-edges;
 *   parallel edges compete whatever their sequences are (a bubble arm beyond max_diff goes if it is weak enough);
 *   an isolated contig is kept by (A) and goes under (B) if it is below the floor;
 *   strand symmetry: the twin of e runs from rc v to rc u, the out-edges of rc v are the twins of the in-edges of v and carry the
 *   same numbers — a strand-closed edge set stays strand-closed under (A), under (B) and under both together.
 * Competitors are found by node id: the copies a node split leaves are different nodes.  Removal is MapGraph.removeEdge (:191-195);
 * nodes stay for the caller's next simplifyGraph.  stats4 (may be NULL) = {candidates, removed_ratio, removed_floor_only, removed}:
 * candidates = the live edges within max_len whose u has out-degree >= 2 and whose v has in-degree >= 2; removed_ratio = the edges
 * removed under (A); removed_floor_only = those removed under (B) that (A) did not remove; removed = the sum of the last two.
 * Coverage is computed for every live edge.  If any window of any live edge is missing from `counts` the map is not this graph's:
 * GK_E_STATE, and the graph is untouched, as with the tips.  Handles as for gk_graph_clip_tips. */
int gk_graph_remove_weak_edges(gk_graph *g, gk_map *counts, uint64_t max_len, uint32_t ratio, uint32_t floor, uint64_t *stats4);

/* ---- contigs: this project's own rule (the reference prints every edge's seq BEFORE a ">abacaba<i>" line, both strands, without
 * the start k-mer: GraphSimplifier.scala:338-347; the host side's Graph::writeContigs is its literal twin and stays) ----
 * The assembly as FASTA text, written on the device.  Integers only.
 * Path.  The path of a live edge e is P(e) = start k-mer ++ seq: n = k + len bases in the 2-bit codes A0 G1 C2 T3 (complement =
 * 3 - code).  The contigs of two edges that meet in a node therefore OVERLAP by that node's k bases.  This is deliberate: a contig
 * is the whole sequence its edge spells, usable on its own, and the overlap is how a reader re-joins contigs at a junction.
 * Strand.  R(e) = the reverse complement of P(e).  P and R are compared lexicographically by code: e is FORWARD if P < R,
 * SELF_TWIN if P == R, REVERSE if P > R.  The twin of an edge has path R(e), so in a strand-closed edge set exactly one edge of
 * every twin pair is forward, and a self_twin edge is its own twin.  The comparison needs no twin lookup: it is well defined after
 * node splits (copies share a k-mer) and after edits that left the set not strand-closed.
 * Classes.  Every live edge falls into exactly one, tested in this order: 1. short: n < min_len (min_len = 0 keeps all);
 * 2. forward, self_twin or reverse, as above.
 * Selection.  strands = 1: the records are the forward and self_twin edges (a reverse edge whose twin is dead is NOT written; the
 * stats show it: in a strand-closed graph forward == reverse).  strands = 2: all three classes (still counted apart).  Any other
 * value: GK_E_INVALID.
 * Text.  Records in ascending edge id.  One record:
 *     >e<id> len=<n>[ cov=<q/100>.<q%100 as two digits>]\n
 *     <the n bases as ACGT text, a '\n' after every line_width bases and after the last base>
 * line_width = 0: the whole sequence on one line.  There is never an empty line, also when line_width divides n.  The cov= field is
 * there iff a count table was passed: q = floor(100 * sum / kmers), with sum and kmers as gk_graph_edge_coverage defines them
 * (len + 1 windows, both end nodes included), computed without overflow.  Windows the table does not hold count 0 and are summed
 * into the stats (over the records); they are no error (gk_graph_edge_coverage's contract, not the tips').  The record of an edge
 * is the same under strands = 1 and strands = 2: always the edge's own path and id.
 * The plan holds what the text is a pure function of (the selected ids, each record's byte offset, q) and the graph's state
 * counter.  The graph is not changed, and must outlive the plan.  After ANY edit of the graph gk_contigs_read and gk_contigs_write
 * return GK_E_STATE; gk_contigs_stats still answers.  `counts` (may be NULL) of another k or context: GK_E_INVALID.  NULL handles:
 * GK_E_INVALID.  A graph without a live edge: an empty text, GK_OK.  A record of 2^32 bytes or more: GK_E_CAPACITY.  On any error
 * *out stays NULL and everything the call allocated is freed.
 * On the device: one wave per live edge compares P with R 64 bases at a time and stops at the first difference; an exclusive scan
 * over the edge ids gives the record offsets; the text is emitted by byte range — a lane writes one aligned 8-byte word, found by a
 * binary search in the offsets — in chunks of 64 MiB through two pinned buffers, the next chunk's kernel beside the current
 * chunk's copy and file write. */
typedef struct gk_contigs gk_contigs;
int gk_graph_contigs_plan(gk_graph *g, gk_map *counts, uint64_t min_len, uint32_t line_width, int strands, gk_contigs **out);
void gk_contigs_destroy(gk_contigs *c);
/* stats9 = {live_edges, short, forward, self_twin, reverse, records, bases, text_bytes, missing_windows}; element 0 = the sum of
 * elements 1..4; bases = the sum of n over the records */
int gk_contigs_stats(const gk_contigs *c, uint64_t *stats9);
/* bytes [offset, offset + min(cap, text_bytes - offset)) of the text; *n = bytes written (n may be NULL); offset > text_bytes:
 * GK_E_INVALID */
int gk_contigs_read(gk_contigs *c, uint64_t offset, char *buf, uint64_t cap, uint64_t *n);
/* the whole text to `path`, through path + ".tmp" and a rename (gk_graph_save's contract: a failed write leaves nothing at path;
 * a path that cannot be opened or written: GK_E_INVALID with the errno text) */
int gk_contigs_write(gk_contigs *c, const char *path);
/* wall ms of the last gk_contigs_read / gk_contigs_write on this handle: {the emit kernels (device events, summed over the chunks),
 * waits for the device-to-host copies, the sink (file writes, or the copy into buf), the whole call} */
int gk_contigs_last_ms(const gk_contigs *c, float *ms4);

/* ---- multi-k: this project's own rule (the reference builds its graph at one k) ----
 * The k2-mers of a graph's contigs added to a count table of a larger k, on the device: the step that lets a graph of a small k
 * seed the table of a large one (assemble at k1, clean, seed, count the reads at k2 beside it, build).  Integers only.
 * Terms.  k1 = the graph's k, k2 = gk_map_k(dst).  P(e), n = k1 + len and the classes are the contigs' (above) with min_len = k2,
 * tested in the same order: short (n < k2), then forward, self_twin, reverse.
 * Rule.  For every forward or self_twin edge that is not short, every k2-window of P(e) — positions 0 .. n - k2 — is oriented
 * exactly as a window of a read is when it is counted at k2 (the hash rule at k2, a tie of the two hashes goes to the reverse
 * complement: FreqFilter.scala:31-32) and update(key, weight, _ + weight) is applied to dst.  In one sentence: dst ends as if every
 * record of gk_graph_contigs_plan(g, NULL, 0, 0, strands = 1) that holds k2 bases had been a read counted `weight` times at k2.
 * What follows from that sentence and is not special-cased: a self_twin path contributes each of its mirrored windows twice (the
 * window at position i and the one at n - k2 - i are reverse complements of each other, hence one key), a palindromic window once
 * per occurrence.  Contigs that meet in a node overlap by k1 < k2 bases: they share no window except where the sequence truly
 * repeats, and a k2-window that crosses a junction node is in no contig and is not added (the reads supply those).  A reverse edge
 * whose twin is dead is NOT added; the stats show it.
 * The graph is not changed and its state counter does not move: contig, GFA and scaffold plans made before the call stay valid.
 * stats6 (may be NULL) = {live_edges, short, forward, self_twin, reverse, windows}: element 0 = the sum of elements 1..4, windows =
 * the sum of n - k2 + 1 over the forward and self_twin edges = the updates applied.
 * NULL handles, handles of different contexts, k2 <= k1, weight == 0 or weight > 65535: GK_E_INVALID, and dst is untouched.  A
 * table that cannot grow: GK_E_CAPACITY as from gk_map_add_counts, with the windows of the chunks before it added.  A graph
 * without a live edge: GK_OK, zeros.  Every combination of key widths works (8-byte graph keys into an 8- or 16-byte table, 16 into
 * 16, k2 = 64 with its tagged slots), into a count-layout table and into a graph-layout one (gk_map_create_for_graph).
 * On the device: one wave per live edge classifies it (the contig plan's comparison); the work item of the emission is a RUN of 16
 * consecutive windows of one contig, so that one long edge spreads over the device: per-edge run counts are scanned, a lane finds
 * its run's edge by binary search in the offsets, builds the first window from the node k-mer and the edge's bases without a
 * per-base loop, rolls window and reverse complement through the rest and stores canonical keys and the weight; the host loop feeds
 * chunks of at most 2^24 windows to the table's insert of counted device keys. */
int gk_map_add_graph_paths(gk_map *dst, gk_graph *g, uint32_t weight, uint64_t *stats6);

/* ---- edge twins: this project's own rule (the reference keeps both strands of everything as unrelated edges) ----
 * Which live edge is the reverse complement of which, by content, exactly.  Integers only; no edge id enters the rule.
 * P(e) and R(e) are the contigs' (above): the start k-mer followed by the sequence, and its reverse complement.
 * C(e)  = the live edges f with P(f) = P(e); e is one of them.   C'(e) = the live edges f with P(f) = R(e).
 * Classes.  Every live edge falls into exactly one, tested in this order:
 *   1. missing:   C'(e) is empty;
 *   2. ambiguous: |C(e)| > 1 or |C'(e)| > 1 — the copies a node split or a span split leaves until simplifyGraph merges them with
 *      their flanks;
 *   3. self:      C'(e) = {e};
 *   4. paired:    C'(e) = {f}, f != e, and twin(e) = f.
 * Twins.  The classes of e and of twin(e) agree and twin(twin(e)) = e: P(f) = R(e) iff P(e) = R(f), since reverse complement
 * is an involution, so e is in C'(f), and C(f) = C'(e), C'(f) = C(e) as sets; e paired means |C(e)| = |C'(e)| = 1, hence |C'(f)| =
 * |C(f)| = 1 with C'(f) = {e}.  A graph is strand-closed iff missing == 0, and free of copies iff also ambiguous == 0.
 * Per id asked for, in the order asked (ids as gk_graph_edge_coverage takes them): cls[i] = GK_TWIN_*, twin[i] = the twin's id for
 * paired, the edge's own for self, 0xFFFFFFFF for missing and ambiguous; a dead or out-of-range id gives GK_TWIN_DEAD and
 * 0xFFFFFFFF.  stats6 = {live_edges, paired, self, missing, ambiguous, key_collisions}, over ALL live edges whatever ids were asked
 * for (n may be 0): live_edges is the sum of the four after it and paired is even.  Any output pointer may be NULL.  The graph is not
 * changed.
 * On the device: the 128-bit path key (below, "the path key") of P(e) and of R(e) — the latter by walking the edge's words
 * backwards with complemented codes — for every live edge; (key of P, id) sorted by radix sort; one wave per live edge finds the
 * runs of key(P(e)) and key(R(e)) by binary search and confirms every candidate by comparing the paths, 64 bases per step.  A
 * candidate with the key but another content is skipped and counted in key_collisions: the answer never rests on the hash. */
#define GK_TWIN_DEAD 0
#define GK_TWIN_PAIRED 1
#define GK_TWIN_SELF 2
#define GK_TWIN_MISSING 3
#define GK_TWIN_AMBIGUOUS 4
int gk_graph_edge_twins(gk_graph *g, const uint32_t *edge_ids, uint64_t n, uint32_t *twin, uint8_t *cls, uint64_t *stats6);

/* ---- the graph as GFA: this project's own rule (GFA 1.0; the reference writes no graph text but its nodes / edges files) ----
 * A GFA segment stands for both strands, the graph holds each strand as an edge: the twins above fold them.
 * Segment.  seg(e) = (twin(e), '-') if e is paired and REVERSE by the contigs' strand rule (P(e) > R(e)); otherwise (e, '+').
 * The segments are the live edges with seg(e) = (e, '+'): of a twin pair the forward edge; self, missing and ambiguous edges are
 * their own segments, so a graph that is not strand-closed, or that holds copies, degrades to a faithful directed picture and
 * loses nothing.  e -> seg(e) is injective over the live edges (a segment s is the image of s itself, and with '-' of twin(s)
 * alone), which is why no two links coincide.
 * Text, in this order:
 *     H\tVN:Z:1.0\n
 *     S\te<id>\t<P(e) as ACGT, one line>\tLN:i:<k + len>[\tKC:i:<sum>]\n        one per segment, ascending id
 *     L\te<a>\t<oa>\te<b>\t<ob>\t<k>M\n                                        one per emitted pair
 * KC is there iff a count table was passed: gk_graph_edge_coverage's `sum` over the len + 1 windows; windows the table does not
 * hold count 0 and are totalled in the stats (over the segments).
 * Pairs.  (e, f) is a pair iff e and f are live and end(e) = start(f) as NODE IDS (copies share a k-mer).  Its line says
 * seg(e) -> seg(f); the overlap is the node's k bases, what the contigs overlap by.  The mirror of (e, f) is (twin f, twin e); it
 * exists iff e and f are each paired or self and end(twin f) = start(twin e).  (e, f) is skipped iff its mirror exists, differs
 * from it and is the smaller id pair (first ids, then second): every mirror pair is written once, a pair that is its own mirror
 * once.  Pairs go in ascending e and, within e, by the first base 0..3 of f (the order of the end node's out-edge slots).
 * stats9 = {live_edges, segments, folded, pairs, links, mirrored, bases, text_bytes, missing_windows}: live_edges = segments +
 * folded, pairs = links + mirrored, bases = the sum of k + len over the segments.
 * The plan, the stale-plan rule (GK_E_STATE from read / write after ANY edit), `counts` (may be NULL; another k or context:
 * GK_E_INVALID), NULL handles, *out on errors and the read / write / last_ms contracts are the contigs' (above).  A graph without
 * a live edge: the header line alone.  A line of 2^32 bytes or more: GK_E_CAPACITY.
 * On the device: the twin pass; one lane per edge sizes its S line and its 0..4 L lines; two scans over the edge ids; the text is
 * emitted by byte range as the contigs' is.  An S line always spells the segment's own path. */
typedef struct gk_gfa gk_gfa;
int gk_graph_gfa_plan(gk_graph *g, gk_map *counts, gk_gfa **out);
void gk_gfa_destroy(gk_gfa *c);
int gk_gfa_stats(const gk_gfa *c, uint64_t *stats9);
int gk_gfa_read(gk_gfa *c, uint64_t offset, char *buf, uint64_t cap, uint64_t *n);
int gk_gfa_write(gk_gfa *c, const char *path);
int gk_gfa_last_ms(const gk_gfa *c, float *ms4);

/* ---- the graph file: MapGraph.write (Graph.scala:232-261) / Graph(file) (:384-390) --------------------------------------
 * The stage boundary between GraphBuilder (GraphBuilder.scala:55-56) and GraphSimplifier (GraphSimplifier.scala:152-153).
 * This project's own format (the reference's is Kryo).  Version 1, every value little-endian.  Header, 128 bytes:
 *     0  8  magic "GKGRAPH\0"             32  8  live nodes stored (Nn)          72  8  gk_graph_id_fingerprint
 *     8  4  version = 1                   40  8  live edges stored (Ne)          80 48  zero
 *    12  4  k (2..31 or 34..64)           48  8  pool bytes (P)
 *    16  8  node id bound                 56 16  gk_graph_checksum (nodes, edges)
 *    24  8  edge id bound (both bounds < 2^32-1: 0xffffffff stays "none")
 * Then these arrays, each starting on an 8-byte boundary (zero padding after an odd count of u32):
 *    node ids u32[Nn] (strictly ascending); node k-mers lo u64[Nn] and, for k >= 34 only, hi u64[Nn] (gk_graph_export_nodes'
 *    encoding); node out-order u32[Nn] (count in bits 0..2, i-th base in bits 4+2i..5+2i); edge ids u32[Ne] (strictly
 *    ascending); edge start node u32[Ne]; edge end node u32[Ne]; edge length u64[Ne]; the pool: for each edge in file order
 *    ceil(len/4) bytes of 2-bit codes packed LSB-first (gk_graph_export_edges' packing), the unused high bits of an edge's last
 *    byte zero.  The file ends where the pool ends.  An edge's first base is the first code of its sequence; in-degrees and the
 *    out-edge table are not stored (the load rebuilds them from the edges).
 * gk_graph_save writes the live nodes and edges only, in ascending id order (the pool compacted in that order): two saves of
 * one graph give the same bytes, and so does a save of its load.  It writes path + ".tmp" and renames it onto path: a failed
 * save leaves nothing at path.  A path that cannot be opened or written: GK_E_INVALID with the errno text.
 * gk_graph_load gives a graph with the saved ids, id bounds, out-edge insertion orders, in-degrees, gk_graph_checksum and
 * gk_graph_id_fingerprint (dead ids stay dead; gk_graph_build_stats reads zeros).  Its checks (after GraphSimplifier.scala:
 * 157-169): ids ascending and in bounds; every edge's start and end live nodes, its length >= 1; one edge per (start node,
 * first base); out-orders that list exactly the bases with an out-edge; pool size = sum of ceil(len/4) and zero padding bits;
 * the last k bases of (start k-mer ++ sequence) = the end node's k-mer; then the recomputed checksum and id fingerprint =
 * the header's.  Any failure: GK_E_FORMAT (GK_E_INVALID if the file cannot be opened or read), *out stays NULL and
 * everything the call allocated is freed.
 * The three values of header bytes 56..79 are part of format version 1, and these formulas are normative for it (restated in
 * tests/checksum_ref.py, which tests/test_graph_file_cpu.py holds to the committed files).  mix64 and G as at gk_map_verify, all
 * arithmetic mod 2^64, (lo, hi) a node's k-mer with hi = 0 for k <= 31:
 *     nodes checksum = sum over the live nodes of mix64(lo ^ mix64(hi ^ 0x13198a2e03707344))
 *     edges checksum = sum over the live edges of h(nbytes), where with s the start node's and t the end node's k-mer
 *         h(0) = mix64(lo_s ^ mix64(hi_s ^ 1)) + 3 * mix64(lo_t ^ mix64(hi_t ^ 2)) + 5 * mix64(len),
 *         h(i + 1) = mix64(h(i) ^ (byte_i + G * (i + 1))),  byte_i = byte i of the edge's ceil(len/4) pool bytes as the file stores
 *         them (the unused high bits of the last byte zero); ids, array order and pool offsets do not enter
 *     id fingerprint = mix64(mix64(node id bound ^ 0x626f756e6473) ^ (edge id bound + G))
 *         + sum over the live nodes of m(m(m(0x6e6f6465, id), lo), hi)
 *         + sum over the live edges of m(m(m(m(m(0x65646765, id), start node id), end node id), first base code), len),
 *         m(a, v) = mix64(a ^ (v + G)). */
int gk_graph_save(gk_graph *g, const char *path);                  /* MapGraph.write, Graph.scala:232-248 */
int gk_graph_load(gk_ctx *ctx, const char *path, gk_graph **out);  /* Graph(file), Graph.scala:384-390 + GraphSimplifier.scala:157-169 */
int gk_graph_k(const gk_graph *g);                                 /* GraphSimplifier.scala:153: k comes from the graph (< 0: error) */
/* wall ms of the last gk_graph_save / gk_graph_load on this context: {file I/O, waits for host<->device copies, device kernels
 * (each phase ends in a sync), the whole call} */
int gk_graph_io_stats(gk_ctx *ctx, float *ms4);

/* ---- paired-end walking: GraphSimplifier.startup (S/scripts/GraphSimplifier.scala:188-318) ------------------------------
 * gk_support = the reference's pathsMap (:209: (edge id, edge id) -> number of read pairs whose walk passes through the two
 * edges one after the other) and badPairs (:211).  It accumulates over calls of gk_graph_walk_pairs. */
typedef struct gk_support gk_support;
int gk_support_create(gk_ctx *ctx, gk_support **out);
void gk_support_destroy(gk_support *s);
int gk_support_size(const gk_support *s, uint64_t *pairs, uint64_t *bad_pairs, uint64_t *walked_orientations);
/* wall ms of the last gk_graph_walk_pairs into this support: {keys cut from the stream, getAll batch, graph snapshot + checks,
 * walks, merge of the per-thread counts} */
int gk_support_last_ms(const gk_support *s, float *ms5);
int gk_support_export(const gk_support *s, uint32_t *e1, uint32_t *e2, uint32_t *count, uint64_t cap, uint64_t *n);   /* unordered */
/* Add n (e1, e2, count) triples and the two counters into s; duplicates in the list add up.  Export, then add into an empty
 * support, reproduces the support.  A count that would pass 2^32-1 fails with GK_E_CAPACITY, and s is then unchanged. */
int gk_support_add(gk_support *s, const uint32_t *e1, const uint32_t *e2, const uint32_t *count, uint64_t n, uint64_t bad_pairs,
                   uint64_t walked_orientations);
/* dst += src on the device (both supports on the same device; dst != src): every (e1, e2) count, bad pairs and walked
 * orientations.  src is unchanged.  Same overflow rule as gk_support_add. */
int gk_support_merge(gk_support *dst, const gk_support *src);
/* :213-247 for the first `npairs` pairs of a `.bin` stream (two records per pair; pairs with a mate shorter than k are
 * skipped, :213).  `positions` = gk_graph_position_map of THIS graph in its current state (GK_E_STATE otherwise).  For each
 * pair the four getAll (:214-217) run as one batch on the device; `annotate` (:192-206) drops an orientation whose mates lie
 * on one edge at a distance inside [range_lo, range_hi]; every (pos1, pos2) is walked as WalkingActor does (:78-125:
 * reachable set bounded by range_hi, paths whose length puts the mates range_lo..range_hi apart) by a device kernel, one wave per pair
 * orientation with its sets in LDS; an orientation whose sets outgrow the LDS is walked by host threads over a snapshot of the
 * graph's edge arrays instead (exact either way); the edge pairs on successful paths are counted once per pair orientation.  The
 * reference's range is 180 to 250 (:146). */
int gk_graph_walk_pairs(gk_graph *g, gk_vmap *positions, gk_support *sup, const uint8_t *bin, size_t nbytes, uint64_t npairs, int range_lo,
                        int range_hi);
/* :272-316: for every node with in- and out-edges the matrix support[in][out]; its connected groups at `cutoff` (genome.cutoff);
 * a group without an out-edge has its in-edge removed, every other group moves to a copy of the node (addNode, replaceEnd,
 * replaceStart); out-edges that no group reached are removed.  Follow with gk_graph_simplify (:318).  Node ids: copies are
 * appended; nodes that existed when the call started are the ones visited (the reference iterates a live map: unspecified). */
int gk_graph_split_by_support(gk_graph *g, const gk_support *sup, int cutoff, uint64_t *removed_edges, uint64_t *new_nodes);

/* ---- reads threaded through the graph: this project's own rule (the reference looks at p1.take(k) and p2.take(k) of a pair,
 * GraphSimplifier.scala:213-217, and drops every other window of both mates) ----
 * Let G be a graph of word size k, PM = gk_graph_position_map of G in its current state, and getAll(w) the positions PM holds for
 * the k-mer w, taken as it is with no canonicalisation (as gk_graph_walk_pairs takes its keys).
 * A record of L bases is threaded iff L >= k + 2; shorter records are skipped.  A threaded record r has two strands, s = r and
 * s = revComplement(r).  On a strand, w_i = s[i .. i+k) for i = 0 .. L-k and P_i = getAll(w_i).  The inner windows are
 * i = 1 .. L-k-1.  Every inner window of every strand falls into exactly one class, tested in this order:
 *   1. off_graph  P_i is empty;
 *   2. repeated   |P_i| >= 2 (the copies a node split leaves share a k-mer; a fresh graph never gets here);
 *   3. on_edge    the one position is an EDGE position;
 *   4. otherwise P_i = { Node v }.
 *        exit:   f = out_edge(v, s[i+k]) is a live edge, |P_{i+1}| = 1, and its position is Edge(f, 1) if len_f > 1, or
 *                Node(end(f)) if len_f = 1;
 *        entry:  |P_{i-1}| = 1, and its position is either Edge(e, len_e - 1) with end(e) = v, or Node(u) with
 *                e = out_edge(u, s[i+k-1]) live, len_e = 1 and end(e) = v;
 *      broken     entry or exit fails;
 *   5. crossing   support[(e, f)] += 1.
 * Counts are per crossing: a read that crosses one node three times adds three (no per-read set is kept, unlike the
 * once-per-orientation rule of the pair walk).  A read and its reverse complement give twin crossings, so a strand-closed graph
 * gets strand-closed support.  bad_pairs and walked_orientations of the support do not move.
 * stats7 (may be NULL) = uint64[7] = {records threaded, inner windows, off_graph, repeated, on_edge, broken, crossings}; element
 * 1 is the sum of elements 2..6.
 * Positions are untrusted: the one position of a window (windows 0 and L-k included: they are neighbours) whose id is out of
 * bounds, or names a dead node or edge, or carries a distance >= len, makes the call return GK_E_STATE, as gk_graph_walk_pairs
 * does.  The positions of a repeated window are not looked at.
 * Stream shapes and errors are gk_reads_correct's / gk_reads_correct_dev's: a host `.bin` stream, ragged or fixed, validated on
 * the host first (GK_E_FORMAT if it ends inside a record) and sent through the device in chunks; or a device buffer of fixed
 * stride 1 + ceil(read_len / 4), where a length byte above read_len is clamped, never followed, and the call fails with
 * GK_E_FORMAT.  Handle errors are gk_graph_walk_pairs': GK_E_KLEN for a position map of another k, GK_E_INVALID for NULL handles
 * or another context.  nreads = 0 is GK_OK with zero stats.  A count that would pass 2^32-1 is GK_E_CAPACITY (gk_support_add's
 * rule).  On ANY error sup is unchanged (the call counts into a support of its own and merges it at the end), and stats7 is
 * zero.  Neither the graph nor the position map changes.  Over N ranks every rank threads its share into its own support and
 * gk_dist_reduce_support sums them: there is no collective of its own.
 * On the device: a workgroup stages 64 records in LDS, a wave takes a record, a lane a window — which is window i of one strand
 * and, reverse-complemented, window L-k-i of the other: two position-map probes per window, the graph is read at node windows
 * only.
 * What it resolves: the split is per node, as the reference's is.  Reads resolve junctions and remove connections that no read
 * spans; a repeat longer than k is an edge between two nodes, which this call does not follow: gk_graph_thread_spans and
 * gk_graph_split_edges_by_spans (below) do, as far as a single read spans the repeat. */
int gk_graph_thread_reads(gk_graph *g, gk_vmap *positions, gk_support *sup, const uint8_t *bin, size_t nbytes, uint64_t nreads, uint64_t *stats7);
int gk_graph_thread_reads_dev(gk_graph *g, gk_vmap *positions, gk_support *sup, const void *dev_records, uint64_t nreads, int read_len, uint64_t *stats7);

/* ---- spans: reads followed across a whole edge.  This project's own rule (the reference resolves per node,
 * GraphSimplifier.scala:272-316, and nothing there follows a read from one node to the next) ----
 * A repeat of r bases, k < r, is an edge m between two nodes: every copy enters it at start(m) and leaves it at end(m).  A read
 * that holds the repeat and a base more on either side, r <= L - 2 for a read of L bases, says which way in belongs to which
 * way out.  gk_graph_thread_spans keeps that.
 * The rule builds on gk_graph_thread_reads': the same records (L >= k + 2), the same two strands, the same position map and
 * getAll, the same window classes.  On one strand of a threaded record, take a crossing at inner window j with key (e_j, f_j), and
 * let m = e_j.  The crossing falls into exactly one class, tested in this order:
 *   1. open         j - len_m < 1: the read began inside m or at its start node;
 *   2. span         window i = j - len_m is a crossing with f_i = m, and every window t with i < t < j is on_edge with the
 *                   position Edge(m, t - i) (with len_m = 1 there is no window between): spans[(e_i, m, f_j)] += 1;
 *   3. interrupted  otherwise.
 * Counts are per occurrence, as crossings are: a read that crosses three nodes in a row over two short edges adds two spans.
 * Twins.  If strand s of a read has crossings at i and j = i + len_m with keys (e, m) and (m, f), the other strand has crossings at
 * L - k - j and L - k - i with keys (twin f, twin m) and (twin m, twin e), len_(twin m) = len_m, and its windows between lie on
 * twin m at the mirrored distances; both i and j are inner windows, so both mirror images are.  A strand-closed graph therefore
 * gets a strand-closed table: the count of (e, m, f) equals that of (twin f, twin m, twin e).
 * stats5 (may be NULL) = uint64[5] = {records threaded, crossings, spans, interrupted, open}; element 1 is the sum of elements
 * 2..4 and equals stats7[6] of gk_graph_thread_reads on the same input.
 * gk_spans is an opaque device table (e, m, f) -> u32 count.  It accumulates over calls.  gk_spans_size: distinct triples and the
 * sum of their counts (either may be NULL).  gk_spans_export: unordered; *n = the triples held, GK_E_CAPACITY (nothing copied) when
 * cap is below it.  gk_spans_add: n (e, m, f, count) records from the host; duplicates in the list add up; export, then add into
 * an empty table, reproduces the table.  A count that would pass 2^32-1 fails with GK_E_CAPACITY (gk_support_add's rule), here
 * and in gk_graph_thread_spans; an id of 2^31 - 1 or more, or a fifth distinct f behind one (e, m) (a node has four out-edges),
 * is GK_E_INVALID.  The table is unchanged on any error.
 * gk_graph_thread_spans / _dev: positions are untrusted, stream shapes and errors are gk_graph_thread_reads' to the letter: a
 * stale position map is GK_E_STATE, one of another k GK_E_KLEN, NULL handles or another context GK_E_INVALID, a host stream that
 * ends inside a record or a device record whose length byte exceeds read_len GK_E_FORMAT; nreads = 0 is GK_OK with zero stats.
 * The call counts into a table of its own and merges it at the end, so on ANY error `spans` is unchanged and stats5 is zero.
 * Neither the graph nor the position map changes.  Edge ids are the graph's at the time of the call; the table holds no state
 * counter.  Over N ranks every rank threads its share, exports, and one rank takes them with gk_spans_add: there is no
 * collective.
 * On the device: k_thread_reads' shape (a workgroup stages 64 records in LDS, a wave takes a record, a lane a window, two
 * position-map probes per window); every window's crossing key stays in LDS, and after a wave barrier the lane that owns a
 * crossing at j reads window j - len_m and the positions between.
 * Where it stops: a repeat that no single read spans, r > L - 2, gives open and interrupted crossings only. */
typedef struct gk_spans gk_spans;
int gk_spans_create(gk_ctx *ctx, gk_spans **out);
void gk_spans_destroy(gk_spans *s);
int gk_spans_size(const gk_spans *s, uint64_t *triples, uint64_t *observations);
int gk_spans_export(const gk_spans *s, uint32_t *e, uint32_t *m, uint32_t *f, uint32_t *count, uint64_t cap, uint64_t *n);   /* unordered */
int gk_spans_add(gk_spans *s, const uint32_t *e, const uint32_t *m, const uint32_t *f, const uint32_t *count, uint64_t n);
int gk_graph_thread_spans(gk_graph *g, gk_vmap *positions, gk_spans *spans, const uint8_t *bin, size_t nbytes, uint64_t nreads, uint64_t *stats5);
int gk_graph_thread_spans_dev(gk_graph *g, gk_vmap *positions, gk_spans *spans, const void *dev_records, uint64_t nreads, int read_len, uint64_t *stats5);
/* The edit.  A live edge m with u = start(m) and v = end(m) is a CANDIDATE iff out-degree(u) = 1, in-degree(v) = 1,
 * p = in-degree(u) >= 2 and q = out-degree(v) >= 2.  Let a_1..a_p be the in-edges of u and b_1..b_q the out-edges of v, both in
 * ascending id, and M[i][j] = (spans(a_i, m, b_j) >= cutoff).  A candidate falls into exactly one class, tested in this order:
 *   1. unequal      p != q;
 *   2. ambiguous    a row or a column of M holds two or more entries;
 *   3. unsupported  a row or a column of M holds none;
 *   4. resolved     M is a permutation.
 * For a resolved m the pair of a_1 keeps m, u and v.  Every other pair (a_i, b_j), taken in ascending a_i, gets a copy u' of u, a
 * copy v' of v, a copy m' of m from u' to v' (same length, first base and bases), replaceEnd(a_i, u') and replaceStart(b_j, v').
 * New ids are appended in order of m's id, then a_i's id: two node ids (u' then v') and one edge id per copy, so the ids are a
 * function of the input.  An edge that is both an in-edge of u and an out-edge of v is allowed (the genome A R B R C: B runs from
 * v back to u; one pair moves its end, another its start).  Different candidates touch disjoint edge ends (the end of an in-edge
 * of u belongs to the one candidate that leaves u, the start of an out-edge of v to the one that enters v), so all edits of a call
 * are independent and are decided on the graph as it was when the call started.  Follow with gk_graph_simplify, which merges m
 * and every copy with its two flanks.
 * Twins.  The rule reads ids only to order, and degrees and counts to decide.  On a strand-closed graph twin m is a candidate iff
 * m is (its in-edges are the twins of m's out-edges and the other way round), its matrix is M transposed under a relabelling of
 * rows and columns, and the four classes are invariant under both; a strand-closed table therefore gives twin decisions, and the
 * pairs of twin m are the twins of the pairs of m.  Which pair keeps the original ids is decided by id order on either strand,
 * so the new graph is strand-closed by sequence, not by id.
 * stats7 (may be NULL) = uint64[7] = {candidates, resolved, unequal, ambiguous, unsupported, new edges, new nodes}; element 0 is
 * the sum of elements 1..4.  cutoff = 0 is GK_E_INVALID.  An edge id bound that would reach 2^31 - 1 (ids in positions are below
 * it), or a node id bound of 2^32, is GK_E_CAPACITY; nothing is edited in either case.  Triples of `spans` that name dead or
 * out-of-range ids, or edges that do not meet as (in-edge of u, m, out-edge of v), are ignored: the table may be older than the
 * graph, and a second call with the same table edits only what the rule still finds.
 * Coverage.  m and its copies hold the same k-mers, and a count table holds each once: gk_graph_edge_coverage reports the full
 * count for each of them (the sum over the copies is the copy number times the true coverage), as it does for node copies.
 * A copy shares m's bases in the sequence pool: after the build nothing rewrites a byte range that an edge owns (the merge of
 * gk_graph_simplify reads its sources and appends; gk_graph_save compacts edge by edge into the file, so the loaded graph has one
 * range per edge; the contigs, the scaffolds and gk_graph_checksum only read).
 * Planning is on the host over the cached snapshot, the edits are device kernels, as gk_graph_split_by_support does it.
 * Where it stops: repeats a single read spans.  Over N ranks every rank threads its share of the reads and gk_dist_reduce_spans
 * sums the tables on every rank before the split. */
int gk_graph_split_edges_by_spans(gk_graph *g, const gk_spans *spans, uint32_t cutoff, uint64_t *stats7);

/* ---- the insert range: this project's own rule (the reference hardcodes `180 to 250`, GraphSimplifier.scala:146, with
 * `160 to 270` commented out beside it, and measures nothing) ----
 * Distances.  `annotate` (:192-206) computes, for a pair whose two first k-mers lie on one edge, (dist2 - dist1) + k: the length
 * of the fragment the pair was read from.  gk_graph_pair_distances keeps those numbers.  A pair has the two orientations
 * gk_graph_walk_pairs walks (:214-219):
 *   orientation 0: P1 = getAll(p1.take(k)), P2 = getAll(p2.take(k).revComplement);
 *   orientation 1: P1 = getAll(p2.take(k)), P2 = getAll(p1.take(k).revComplement);
 * a pair with a mate shorter than k gives none (:213).  With max_dist = bins - 1, every orientation falls into exactly one
 * class, tested in this order (integers only):
 *   unplaced    P1 or P2 is empty;
 *   repetitive  |P1| > 16 or |P2| > 16: the lists are not looked at (the work of one lane is bounded; a fresh graph holds a k-mer
 *               once and never gets here, the node copies of a split can);
 *   apart       C = the (a, b) with a in P1, b in P2, both EDGE positions with the same edge id; C is empty;
 *   ambiguous   |C| >= 2;
 *   reversed    for the one (a, b), on edge e: D = dist(b) - dist(a) + k, signed; D < k (b does not lie after a: what an
 *               outward-facing mate-pair library gives.  It is reported, not interpreted);
 *   beyond      D > max_dist;
 *   near_end    dist(a) + max_dist - k >= len_e: had the fragment been max_dist long, its far k-mer would lie off the edge;
 *   counted     none of the above: hist[D] += 1.
 * near_end removes the truncation bias: an edge shows a fragment only if both its ends fit, so short fragments are seen wherever
 * the near mate lands and long ones only far from the edge's end.  After the test every D <= max_dist is observable from exactly
 * the same positions, and short fragments on short edges do not skew the histogram.  So `bins` is part of the rule: it should
 * exceed the largest fragment expected by little (the tools' --max-insert), not by much — an edge shorter than bins - 1 - k
 * counts nothing.
 * hist = uint64[bins], 2 <= bins <= 65536: THIS call's pairs only (callers add batches).  classes = uint64[9] = {orientations,
 * unplaced, repetitive, apart, ambiguous, reversed, beyond, near_end, counted}; element 0 is the sum of the other eight = twice
 * the pairs that were not skipped.  Handles, stream shapes and errors are gk_graph_walk_pairs': `positions` =
 * gk_graph_position_map of THIS graph in its current state on the graph's context (GK_E_KLEN for another k, GK_E_STATE if a
 * position names nothing live in this graph), the first `npairs` pairs of a `.bin` stream (GK_E_FORMAT if it ends inside a
 * pair).  Neither the graph nor the position map changes.  On the device: one lane per orientation over the getAll batch's CSR,
 * a histogram per workgroup in LDS for D < 4096 (one global atomic per non-empty bin at the end), global atomics beyond. */
int gk_graph_pair_distances(gk_graph *g, gk_vmap *positions, const uint8_t *bin, size_t nbytes, uint64_t npairs, uint32_t bins, uint64_t *hist,
                            uint64_t *classes);
/* The range.  Pure host code: no context, no device (gk_spectrum_cutoff's kind).  n = the sum of hist, cum(D) = hist[0] + .. +
 * hist[D].  n < max(min_observations, 1): GK_OK with *range_lo = *range_hi = *median = 0, "no estimate" (callers fall back to
 * the reference's 180..250 and say so: the convention of a spectrum without a valley).  Otherwise
 *   *range_lo = the smallest D with 1000 * cum(D) >  trim_permille * n,
 *   *range_hi = the smallest D with 1000 * cum(D) >= (1000 - trim_permille) * n,
 *   *median   = the smallest D with    2 * cum(D) >= n,
 * compared exactly (128-bit products).  trim_permille = 0 gives the smallest and the largest occupied bin; trim_permille > 499, a
 * NULL hist or bins outside 2..65536: GK_E_INVALID.  Any output pointer may be NULL.  The callers' defaults, trim_permille = 25
 * (the central 95 %) and min_observations = 1000, are choices, not measurements.  The result is in annotate's unit, fragment
 * length; the walks of gk_graph_walk_pairs measure between the mates' first k-mers and the tools pass the range as it is, as the
 * reference passes its `180 to 250` to both (:146, :199, :104). */
int gk_insert_range(const uint64_t *hist, uint32_t bins, uint32_t trim_permille, uint64_t min_observations, uint32_t *range_lo, uint32_t *range_hi,
                    uint32_t *median);
/* gk_graph_pair_distances over the ranks: every rank passes ITS share of the pairs and its replica of the graph with that
 * replica's position map; afterwards every rank holds the sums of hist and classes over all ranks (`bins` the same on every
 * rank).  COLLECTIVE: two all-reduces (uint64 max: a status word; uint64 sum: hist and classes as one array).  gk_dist_spectrum's
 * failure contract: a rank whose local pass failed (a NULL graph or position map included) still takes part and says so in the
 * status word: every rank then returns an error, nobody waits, and the handle stays usable.  A NULL `d`, `hist` or `classes`, or
 * bad `bins`, is GK_E_INVALID on the rank that passes it, before the collective. */
int gk_dist_pair_distances(gk_dist *d, gk_graph *g, gk_vmap *positions, const uint8_t *bin, size_t nbytes, uint64_t npairs, uint32_t bins, uint64_t *hist,
                           uint64_t *classes);

/* ---- scaffold links: this project's own rule (the reference ends at the split and the contigs; nothing there orders two edges
 * that the graph does not connect, or connects only through a tangle) ----
 * The orientations gk_graph_pair_distances counts as `apart`, the mates on two different edges, are the scaffolding evidence.
 * gk_graph_pair_links keeps them.  Orientations are exactly gk_graph_pair_distances':
 *   orientation 0: P1 = getAll(p1.take(k)), P2 = getAll(p2.take(k).revComplement);
 *   orientation 1: P1 = getAll(p2.take(k)), P2 = getAll(p1.take(k).revComplement);
 * a pair with a mate shorter than k gives none.  P(e) = start k-mer ++ seq is the path of edge e, k + len_e bases.  An orientation
 * whose placements are a = Edge(e, da) and b = Edge(f, db) would spell a fragment that starts at base da of P(e) and ends after
 * base db + k of P(f): D = u + G bases, where G is the number of bases between the end of P(e) and the start of P(f) (G = -k
 * when f leaves e's end node: the two paths share the node's k-mer) and
 *   u = (len_e + k - da) + (db + k)
 * is the number of bases the fragment needs on the two edges.  Every orientation falls into exactly one class, tested in this
 * order (integers only):
 *   unplaced    P1 or P2 is empty;
 *   repetitive  |P1| >= 2 or |P2| >= 2: the lists are not looked at (a fresh graph holds a k-mer once and never gets here, the
 *               node copies of a split can);
 *   at_node     either single position is a NODE position;
 *   same_edge   e == f: that case is gk_graph_pair_distances' business;
 *   short_edge  k + len_e < min_len or k + len_f < min_len (min_len in contig bases, as gk_graph_contigs_plan's; 0 keeps all);
 *   too_far     u > max_span;
 *   linked      links[(e, f)].count += 1 and links[(e, f)].sum_u += u.
 * The table stores sum_u, not a gap, so the device rule needs no library parameter: a caller that knows the fragment median M
 * reads the mean gap of a link as M - floor(sum_u / count), signed.  sum_u adds up mod 2^64.
 * Twins.  Orientation 1 of a pair is the same fragment read on the other strand.  If orientation 0 places p1.take(k) at base da of
 * P(e) and p2.take(k).revComplement at base db of P(f), then on the twin edges (P(twin x) = revComplement of P(x), same length)
 * p2.take(k) lies at base len_f - db of P(twin f) and p1.take(k).revComplement at base len_e - da of P(twin e): orientation 1
 * lands on (twin f, twin e) with u' = (len_f + k - (len_f - db)) + ((len_e - da) + k) = u.  Both distances stay inside 1 .. len - 1,
 * so both orientations are EDGE positions or neither is, and the same two lengths meet min_len.  A strand-closed graph therefore
 * gets a strand-closed link table: count and sum_u of (e, f) equal those of (twin f, twin e).
 * classes8 = uint64[8] = {orientations, unplaced, repetitive, at_node, same_edge, short_edge, too_far, linked}; element 0 is the
 * sum of the other seven.
 * gk_graph_pair_links: handles, stream shapes (a ragged or fixed host `.bin` stream, its first `npairs` pairs) and errors are
 * gk_graph_pair_distances': GK_E_KLEN for a position map of another k, GK_E_STATE for a stale one (a position that names nothing
 * live in this graph: checked before the kernel reads an edge length), GK_E_FORMAT for a stream that ends inside a pair,
 * GK_E_INVALID for NULL handles or another context.  It accumulates over calls: it counts into a table of its own and merges
 * that at the end, as gk_graph_thread_reads does, so on ANY error `links` is unchanged and classes8 is zero.  A count that would
 * pass 2^32-1 is GK_E_CAPACITY (gk_support_add's rule), here and in gk_links_add.  Neither the graph nor the position map
 * changes.  Edge ids are the graph's at the time of the call: the table holds no state counter and is MEANINGLESS after a graph
 * edit; make a new one.  Over N ranks every rank links its share and gk_dist_reduce_links sums the tables on every rank.
 * On the device: one lane per orientation over the getAll batch's CSR, class counts by ballot, one insert per linked lane into an
 * open-addressed (e << 32 | f) table with a u32 count plane and a u64 sum plane, sized before the launch for one link per
 * orientation at load <= 0.5. */
typedef struct gk_links gk_links;
int gk_links_create(gk_ctx *ctx, gk_links **out);
void gk_links_destroy(gk_links *l);
int gk_graph_pair_links(gk_graph *g, gk_vmap *positions, gk_links *links, const uint8_t *bin, size_t nbytes, uint64_t npairs, uint64_t min_len,
                        uint64_t max_span, uint64_t *classes8);
/* distinct (e, f) and the sum of their counts (either may be NULL) */
int gk_links_size(const gk_links *l, uint64_t *links, uint64_t *observations);
/* unordered; *n = the links held, GK_E_CAPACITY (nothing copied) when cap is below it */
int gk_links_export(const gk_links *l, uint32_t *e1, uint32_t *e2, uint32_t *count, uint64_t *sum_u, uint64_t cap, uint64_t *n);
/* Add n (e1, e2, count, sum_u) records; duplicates in the list add up.  Export, then add into an empty table, reproduces the
 * table.  A count that would pass 2^32-1 fails with GK_E_CAPACITY, and l is then unchanged.  0xffffffff is not an edge id. */
int gk_links_add(gk_links *l, const uint32_t *e1, const uint32_t *e2, const uint32_t *count, const uint64_t *sum_u, uint64_t n);

/* ---- links and spans over the ranks: this project's own rules ----------------------------------------------------------------
 * Links and spans are taken on the FINAL graph: after gk_graph_split_by_support and gk_graph_simplify, and for later resolve
 * rounds after gk_graph_split_edges_by_spans too.  The replicas of such a graph hold the same edges under different ids, and their
 * copies share k-mers, so gk_dist_reduce_support's numbering by (start k-mer, first base) cannot name them.  These two collectives
 * number the edges by what they spell.
 * The path key.  P(e) = start k-mer ++ seq, k + len bases.  With mix64 the 64-bit finalizer
 *     mix64(x): x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33
 * and fold(a, v) = mix64(a ^ (v + 0x9e3779b97f4a7c15)), all arithmetic mod 2^64:
 *     word j of e, j = 0 .. ceil(len / 32) - 1: the bases seq[32j .. 32j + 31], base 32j + i at bits 2i and 2i + 1 (codes A0 G1
 *         C2 T3), the bases past the end of seq zero — counted from the edge's own first base, wherever the edge lies in memory;
 *     t(j) = word j ^ mix64(j + 0x70617468776f7264);   S1 = sum over j of mix64(t(j));   S2 = sum of mix64(t(j) ^ 0x7365636f6e64);
 *     h1 = fold(fold(fold(fold(0x7061746831, S1), lo), hi), len),   h2 = the same from 0x7061746832 and S2,
 *         (lo, hi) the start k-mer's two words (gk_graph_nodes_by_id's); an h1 of 2^64 - 1 becomes 2^64 - 2.
 * (h1, h2) is a function of the path alone, and the sums over words are what lets the device hash a long edge in pieces.  The
 * canonical order of the live edges is ascending (h1, h2) — the length is no third sort key: it is folded into both hashes, so
 * two paths of different length share a key only by a 128-bit collision, and would then count as duplicates.  Two live edges with equal keys are DUPLICATES: neighbours in the
 * order, told apart by nothing a replica agrees on.  They are no error in themselves — every k-mer of such an edge has two
 * positions, gk_graph_pair_links classes it `repetitive` and gk_graph_thread_spans follows no read through it, so no table these
 * calls made names one — but a record that does name one, or a dead edge, fails the reduce with GK_E_STATE.  The replicas'
 * FINGERPRINT is mix64(live edges ^ 0x6c697665) + the sum over live edges of mix64(h1 ^ mix64(h2 + 0x66696e676572)): equal on two
 * replicas iff they hold the same multiset of paths (up to a 128-bit collision).  tests/pathkey_ref.py restates all of this.
 * gk_dist_reduce_links.  Every rank holds a replica of g and has linked ITS share of the pairs into `links`; afterwards every
 * rank's table holds the element-wise sum over all ranks — counts added (a sum past 2^32-1: GK_E_CAPACITY), sum_u added mod 2^64 —
 * keyed by THIS rank's edge ids.  The contract is gk_dist_reduce_support's, step for step: the ranks agree on every rank's status
 * and on equal fingerprints (GK_E_STATE otherwise) before any payload moves; a record goes to its owner rank by a hash of the
 * canonical (e1, e2), one all-to-all of (key u64, count u32, sum_u u64) planes; after the owners' merge the ranks agree on "no
 * count passed 2^32-1" and on the shard sizes, every shard goes to every rank, the keys go back to this replica's ids, and after
 * the rebuild the ranks agree once more before anything is swapped in.  If any of this fails on any rank, every rank returns an
 * error, every table is unchanged, no rank is left in a receive and the handle stays usable.  world == 1: only the checks run.
 * gk_dist_reduce_spans: the same for (e, m, f) -> count.  The owner is a hash of the canonical (e, m), so the at most four
 * out-edges behind one (e, m) meet at one owner; more than four over the ranks is GK_E_STATE.
 * Both: COLLECTIVE, world <= 64, the graph is only read.  The joins, chains and scaffold text that follow are per rank and follow
 * the rank's own ids: ranks agree on the SET of joins, chains and records, not on their order. */
int gk_dist_reduce_links(gk_dist *d, gk_graph *g, gk_links *links);
int gk_dist_reduce_spans(gk_dist *d, gk_graph *g, gk_spans *spans);
/* Joins.  A link is SUPPORTED iff count >= min_support.  (e, f) is a JOIN iff it is the only supported link out of e and the only
 * supported link into f.  The joins come in ascending e1 (an e1 occurs at most once, so the order is total), with their count and
 * sum_u.  stats5 (may be NULL) = uint64[5] = {links, supported, joins, edges with >= 2 supported successors, edges with >= 2
 * supported predecessors}.  *n = joins; cap below it is GK_E_CAPACITY with *n and stats5 set and nothing copied.  On the device:
 * one pass over the slots counts successors and predecessors per edge id, one lane per edge id flags the joins, a scan and a
 * compaction in id order emit them. */
int gk_links_joins(const gk_links *l, uint32_t min_support, uint32_t *e1, uint32_t *e2, uint32_t *count, uint64_t *sum_u, uint64_t cap, uint64_t *n,
                   uint64_t *stats5);
/* Chains.  Pure host code: no context, no device (gk_insert_range's kind).  Input: a join list, in which no id occurs twice as e1
 * or twice as e2 (GK_E_INVALID otherwise); such joins form disjoint paths and cycles.  A chain is a maximal path in join order; a
 * cycle is a chain that starts at its smallest edge id, and is counted in *ncycles.  Edges in no join are not listed.  Chains come
 * in ascending order of first member: chain i is members[chain_off[i] .. chain_off[i + 1]), so chain_off holds chains_cap + 1
 * words.  n joins give at most n chains of at most 2n members together; less room than needed is GK_E_CAPACITY with *nchains and
 * *ncycles set and nothing written. */
int gk_scaffold_chains(const uint32_t *e1, const uint32_t *e2, uint64_t n, uint32_t *members, uint64_t members_cap, uint64_t *chain_off, uint64_t chains_cap,
                       uint64_t *nchains, uint64_t *ncycles);

/* ---- scaffolds: this project's own rule (the reference has no links and writes no scaffolds) ----
 * The chains as FASTA text, written on the device: junctions inside the graph joined, gaps N-filled, one strand per chain.
 * Integers only.
 * Input.  A chain list in gk_scaffold_chains' shape: chain c is members[chain_off[c] .. chain_off[c + 1]), chain_off[0] = 0, so
 * `members` holds chain_off[nchains] edge ids.  `gap` is parallel to `members`: gap[j] is the estimated number of bases between
 * members[j] and members[j + 1] of the same chain (the tools pass mid - floor(sum_u / count) of the join, which may be negative);
 * the entry at a chain's last member is ignored.  A cycle therefore comes out open, cut where gk_scaffold_chains starts it.
 * Paths.  P(e) = start k-mer ++ seq, k + len_e bases, as in the contig rule.
 * Junction.  Every junction between consecutive members e, f falls into exactly one class, tested in this order:
 *   adjacent  e_end[e] == e_start[f], the same node ID (copies of a node that share a k-mer are different nodes): the two paths
 *             share that node's k-mer, so f contributes bases k .. of P(f) and nothing goes between; the gap is not looked at;
 *   gapped    anything else: a run of max(gap, min_gap) bases N, then all of P(f).  A gap below min_gap counts as CLAMPED (it is
 *             gapped too).  Overlaps are not looked for here: a negative gap is clamped like any other, unless the caller passes
 *             the overlaps of gk_graph_overlap_gaps to gk_graph_scaffolds_plan_overlaps (below, "overlap detection").
 * Sequence.  S(c) = P(first member) followed by what every junction adds, over the codes A0 G1 C2 T3 N4; n = its length.
 * Strand.  R(S) = S reversed with code c mapped to 3 - c for c < 4, and 4 staying 4.  A chain is FORWARD if S < R
 * lexicographically by code, SELF_TWIN if S == R, REVERSE otherwise.  No twin lookup is needed, for the reason the contig rule
 * gives.  On a strand-closed graph with a strand-closed link table (see "scaffold links", Twins) the join (e, f) comes with the
 * join (twin f, twin e) of the same count and sum_u, hence the same gap; a chain (e1 .. em) comes with (twin em .. twin e1).  Its
 * junction (twin e[i+1], twin e[i]) is adjacent iff (e[i], e[i+1]) is: end(e[i]) = start(e[i+1]) = v means start(twin e[i]) =
 * end(twin e[i+1]) = the node of v's reverse complement.  P(twin x) is the reverse complement of P(x), an adjacent junction drops
 * the same k bases from either side and an N run reads the same backwards, so the twin chain's sequence is R(S): exactly one chain
 * of such a pair is forward, or both are the same self_twin chain.
 * Selection.  strands = 1: the forward and self_twin chains (a reverse chain whose twin chain is absent is NOT written; the stats
 * show it).  strands = 2: all chains.  Other values: GK_E_INVALID.  singletons != 0: every live edge that is a member of no given
 * chain is written too, with min_len and strands applied exactly as gk_graph_contigs_plan applies them.  Chain members are never
 * dropped for length.
 * Text.  The selected chains in input order, then the singletons in ascending edge id.  A chain's record:
 *     >s<c> len=<n> contigs=<m> gaps=<N bases>\n
 *     <the n bases as ACGTN text, wrapped as contigs are: a '\n' after every line_width bases (0: one line) and after the last>
 * c is the chain's index in the input, so a record is the same under both values of `strands`; m = its members.  A singleton's
 * record is byte for byte the contig rule's without cov=: ">e<id> len=<n>\n" and the wrapped bases.  There is never an empty line.
 * Errors, all found on the device in one pass before any kernel reads a member's length.  GK_E_INVALID: a member id at or above
 * the edge id bound, or dead; an edge that occurs twice, in one chain or in two; an empty chain or a chain_off that does not
 * ascend; min_gap outside 1 .. 2^31-1; a used gap above 2^31-1; strands not 1 or 2; line_width above 2^31-1; NULL handles or
 * arrays.  GK_E_CAPACITY: a record of 2^32 bytes or more.  nchains = 0 is legal; with singletons the text is then
 * gk_contigs_read's of the same graph without a count table.  On any error *out stays NULL and everything allocated is freed.
 * The graph is not changed and must outlive the plan; after ANY edit of it gk_scaffolds_read and gk_scaffolds_write return
 * GK_E_STATE, while stats and segments still answer.
 * min_gap has no measured value: the tools and the Python side pass 10, the customary shortest N run, as a choice.
 * On the device: one lane per member claims its edge (a compare-and-swap on an owner word per edge finds duplicates) and decides
 * its junction; a scan over the segment lengths places every segment; one wave per chain compares S with R 64 bases at a time,
 * a lane finding its base by a binary search in the chain's segments; two more scans and a compaction give record -> (segments,
 * byte offset); the text is emitted by byte range as contigs are, the segment of a lane's first base found by a binary search.
 * Not there: cov= on scaffold records, a collective over ranks (links are per rank). */
typedef struct gk_scaffolds gk_scaffolds;
int gk_graph_scaffolds_plan(gk_graph *g, const uint32_t *members, const uint64_t *chain_off, uint64_t nchains, const int64_t *gap, int64_t min_gap,
                            uint64_t min_len, uint32_t line_width, int strands, int singletons, gk_scaffolds **out);
void gk_scaffolds_destroy(gk_scaffolds *s);
/* stats13 = {chains, chain_forward, chain_self_twin, chain_reverse, singletons, records, members, adjacent, gapped, clamped,
 * n_bases, bases, text_bytes}: chains = the sum of the three after it; singletons = singleton records; records = chain records +
 * singletons; members .. n_bases are over the chain records (members = their pieces, adjacent + gapped = members - chain
 * records, clamped <= gapped, n_bases = their N); bases = the sum of n over all records.  With overlaps
 * (gk_graph_scaffolds_plan_overlaps) the identity becomes adjacent + gapped + overlapped = members - chain records, `overlapped`
 * being gk_scaffolds_overlap_stats' first number */
int gk_scaffolds_stats(const gk_scaffolds *s, uint64_t *stats13);
/* gk_contigs_read's, gk_contigs_write's and gk_contigs_last_ms' contracts, for this text */
int gk_scaffolds_read(gk_scaffolds *s, uint64_t offset, char *buf, uint64_t cap, uint64_t *n);
int gk_scaffolds_write(gk_scaffolds *s, const char *path);
int gk_scaffolds_last_ms(const gk_scaffolds *s, float *ms4);
/* The layout of the records, one row per piece of an edge in text order: the record's index in the text, the edge id, the first
 * base of the piece in the record's sequence, the bases written, and the bases of P(edge) skipped before them (0, k after an
 * adjacent junction, or o after an overlapped one).  N runs are the bases between rows.  *n = rows = members + singletons of the stats; cap below it is
 * GK_E_CAPACITY with *n set and nothing copied. */
int gk_scaffolds_segments(const gk_scaffolds *s, uint64_t *record, uint32_t *edge, uint64_t *first, uint64_t *bases, uint32_t *skipped, uint64_t cap,
                          uint64_t *n);

/* ---- gap filling: this project's own rule (the reference has no scaffolds) ----
 * A stage between gk_scaffold_chains and gk_graph_scaffolds_plan: where the graph holds exactly one path of the right length
 * between two consecutive members of a chain, that path's edges become members.  The junction is then a run of adjacent
 * junctions, which the scaffold rule joins on their k bases: no N is written there.  Integers only.  The graph is not edited.
 * Input.  members, chain_off, nchains and gap exactly as gk_graph_scaffolds_plan takes them; tol (bases) 0 .. 2^31-1; max_edges
 * 1 .. GK_FILL_MAX_EDGES; max_paths 1 .. GK_FILL_MAX_PATHS.
 * Path.  Take a junction (e, f) of consecutive members with e_end[e] != e_start[f] and G = its gap.  A path is a sequence x1..xm
 * of live edges, 1 <= m <= max_edges, with e_start[x1] == e_end[e] and e_end[x(i)] == e_start[x(i+1)] throughout; equality is by
 * node id, as the scaffold rule's `adjacent` is.  An edge may occur twice on a path.  (A live edge that gk_graph_replace_start has
 * displaced from its start node's out-edge word, as the reference's map does, is on no path, from either side.)  Its sum is S = len(x1) + .. + len(xm)
 * (every edge has len >= 1) and its gap length is L = S - k: the bases between the end of P(e) and the start of P(f) when the path
 * ends in e_start[f].  L < 0 (S < k) is legal: the adjacent junctions of the filled chain spell the overlap correctly.
 * With B = G + tol + k:
 *   T_fwd  the set of all paths from e_end[e] with S <= B (prefix-closed);
 *   T_bwd  the set of all edge sequences y1..ym, 1 <= m <= max_edges, S <= B, that run backwards from e_start[f]:
 *          e_end[y1] == e_start[f], e_start[y(i)] == e_end[y(i+1)];
 *   hit    a path that ends in e_start[f] with G - tol <= L <= G + tol.  A hit lies in T_fwd, and reversed in T_bwd (it starts
 *          in e_end[e] there), so the hits are the same from either side.
 * Classes of a junction, tested in this order (jclass is parallel to members, as gap is; GK_FILL_LAST at a chain's last member):
 *   adjacent   as in the scaffold rule; nothing is searched, the gap is not looked at;
 *   overflow   |T_fwd| > max_paths AND |T_bwd| > max_paths.  Set sizes, not a traversal: any implementation decides it alike.
 *              Both sides, because the twin junction (twin f, twin e) has the mirrored trees: with one side only a chain could be
 *              filled and its twin chain not;
 *   none       no hit; B < 1 is this class (nothing is searched);
 *   ambiguous  two or more hits.  A bubble between e and f stays N: no hit is preferred over another;
 *   unique     exactly one hit: a candidate.
 * After all junctions are classed, a candidate is SHARED when any edge of its path is a member of any input chain, lies on
 * another candidate's path, or occurs twice on its own path: every candidate that touches a contested edge loses, whatever the
 * order (uses are counted per edge first, then tested).  Every other candidate is FILLED.  jclass holds shared or filled, never
 * unique.
 * Output.  The chains in input order; a filled junction e, f becomes e, x1..xm, f; each new junction gets gap -k (the scaffold
 * plan never looks at it: it is adjacent); every other junction keeps its gap, and so does the unused entry at a chain's last
 * member.  out_chain_off holds nchains + 1 words.  jlen[j] = L where jclass[j] is shared or filled, else 0.  *n_members = the
 * members written = chain_off[nchains] + filler_edges; it never exceeds the live edges, since no edge is written twice.
 * members_cap below it is GK_E_CAPACITY with *n_members and stats10 set and nothing copied.
 * stats10 = {junctions, adjacent, overflow, none, ambiguous, shared, filled, filler_edges, filler_bases, searched_backward}:
 * element 0 is the sum of the next six; filler_edges / filler_bases = the sum of m / of S over the filled junctions;
 * searched_backward = the junctions whose forward tree overflowed (informational, and not strand-symmetric).
 * Twins.  On a strand-closed graph, a path x1..xm from e_end[e] to e_start[f] comes with (twin xm .. twin x1) from
 * e_end[twin f] to e_start[twin e], of the same lengths.  So T_fwd of (e, f) is T_bwd of (twin f, twin e) reversed, and the
 * hits of one are the twins of the hits of the other: with the same G, tol and bounds the two junctions fall into the same
 * class (overflow takes both trees, hence is symmetric), and a unique hit is the twin of the other's.  An edge is contested
 * iff its twin is (the uses mirror), so a chain and its twin chain (gk_graph_scaffolds_plan, Strand) are filled alike: the
 * filled chains are again a chain and its twin chain, and strands = 1 still writes exactly one of them.
 * Errors.  GK_E_INVALID: the scaffold plan's member and chain errors (an id at or above the bound, or dead; an edge twice; an
 * empty chain; a chain_off that does not ascend); a parameter out of range; NULL handles or arrays; |G| above 2^31-1 at a junction
 * that is not adjacent.  All are found on the device before a kernel reads a member's length.  On any error nothing is written
 * (GK_E_CAPACITY above is the one exception: it sets *n_members and stats10).  The graph is never changed.
 * The defaults the tools and the Python side pass (max_edges 16, max_paths 256, tol = half the width of the insert range) are
 * choices, not measurements.
 * On the device: the scaffold plan's check (one lane per member claims its edge's owner word) and one lane per junction for
 * adjacent / B < 1; a scan compacts the junctions to search.  k_fill_search: one wave per junction, the tree in LDS (edge, parent
 * index, running S per entry; GK_FILL_MAX_PATHS entries of 10 bytes = 10 KiB per wave), built level by level: lanes take frontier
 * entries and read the end node's four out-edge words (the start node's in-edge list for the backward tree), live children
 * within B are appended by ballot and prefix count, hits are counted by ballot; a direction stops the moment its count passes
 * max_paths, and the backward tree runs only then.  A unique hit is unwound through the parent indices into HBM in path order.
 * No global atomics in the search.  Then one atomic add per path edge (uses), one lane per junction (shared / filled), a scan
 * over the per-member output counts and a write kernel; one read-back at the end.  The in-edge lists are built on every call
 * (two passes over the edges and a scan over the nodes), needed or not.
 * Not there: a collective over ranks. */
#define GK_FILL_MAX_EDGES 64        /* a path's edges: one lane each when a hit is unwound */
#define GK_FILL_MAX_PATHS 1024      /* entries of one wave's LDS tree: 4 waves x 10 KiB = 40 KiB per workgroup, 4 workgroups per CU */
enum { GK_FILL_LAST = 0, GK_FILL_ADJACENT = 1, GK_FILL_OVERFLOW = 2, GK_FILL_NONE = 3, GK_FILL_AMBIGUOUS = 4, GK_FILL_SHARED = 5, GK_FILL_FILLED = 6 };
int gk_graph_fill_gaps(gk_graph *g, const uint32_t *members, const uint64_t *chain_off, uint64_t nchains, const int64_t *gap, uint64_t tol,
                       uint32_t max_edges, uint32_t max_paths, uint32_t *out_members, int64_t *out_gap, uint64_t members_cap, uint64_t *out_chain_off,
                       uint8_t *jclass, int64_t *jlen, uint64_t *n_members, uint64_t *stats10);

/* ---- overlap detection: this project's own rule (the reference has no scaffolds) ----
 * A stage between gk_graph_fill_gaps (or gk_scaffold_chains) and the scaffold plan: where the paths of two consecutive chain
 * members overlap, exactly, by a number of bases that the gap estimate allows, the plan writes those bases once instead of twice
 * with min_gap bases N between them.  The commonest cause is a coverage dip: w consecutive k-mers (1 <= w <= k - 2) missing from
 * the count table leave two contigs whose paths share k - 1 - w bases, no graph path between them (gk_graph_fill_gaps: none),
 * and a link whose gap is near -(k - 1 - w).  Integers only.  The graph is not edited and the chains are not rewritten.
 * Input.  members, chain_off, nchains and gap exactly as gk_graph_scaffolds_plan takes them; tol (bases) 0 .. 2^31-1; min_overlap
 * 1 .. GK_OVERLAP_MAX; max_overlap min_overlap .. GK_OVERLAP_MAX.  GK_OVERLAP_MAX = 127 is a bound of the implementation, not a
 * measurement: 127 = 2 * 64 - 1 bases, so a side fits four 64-bit words of 2-bit codes and an overlap fits the plan's one-byte skip
 * column; it is also the longest overlap two edges at k = 64 can have without sharing a whole k-mer of sequence.  (In an unedited
 * graph two different edges share no interior k-mer, so overlaps are below k; node copies that share a k-mer give exactly k; by-id
 * edits can give more.)
 * Paths.  P(e) = start k-mer ++ seq, as in the scaffold rule; |P(e)| = k + len_e.
 * Candidates.  Take a junction (e, f) of consecutive members that is not adjacent (e_end[e] != e_start[f], by node id, as in the
 * scaffold rule) and G = its gap.  The candidates are the o in lo .. hi with
 *   lo = max(min_overlap, -G - tol)
 *   hi = min(max_overlap, -G + tol, |P(e)| - 1, |P(f)| - 1):
 * neither member may be contained in the other, and f always adds at least one base.
 * Hit.  o is a hit when the last o bases of P(e) equal the first o bases of P(f), exactly.
 * Classes of a junction, tested in this order (jclass is parallel to members, as gap is):
 *   last          at a chain's last member;
 *   adjacent      as in the scaffold rule; nothing is searched, the gap is not looked at;
 *   out_of_range  lo > hi; nothing is searched.  Every ordinary positive gap lands here;
 *   none          no hit;
 *   ambiguous     two or more hits.  A periodic end stays N: no hit is preferred over another;
 *   overlap       exactly one hit.
 * Output.  overlap[j] = the hit where jclass[j] is overlap, else 0.  stats7 = {junctions, adjacent, out_of_range, none, ambiguous,
 * overlap, overlap_bases}: element 0 is the sum of the next five, overlap_bases the sum of overlap[].
 * Why exact.  If the last o bases of P(e) are the first o bases of P(f), the sequence built so far, which ends with all of P(e),
 * followed by bases o .. of P(f), ends with all of P(f).  The next junction's overlap, however long (it may exceed what f
 * contributed), is therefore an overlap with the text actually written, and nothing has to choose between two spellings.  With
 * mismatches allowed a rule would have to say whose bases are written; exactness avoids that.
 * Twins.  P(twin x) is the reverse complement of P(x), so the last o bases of P(e) equal the first o of P(f) iff the last o bases
 * of P(twin f) equal the first o of P(twin e).  The two path lengths are the same for the junction (twin f, twin e), and on a
 * strand-closed link table so is G (see "scaffold links", Twins); adjacent mirrors too (gk_graph_scaffolds_plan, Strand).  Hence lo,
 * hi and the set of hits are the same: a chain and its twin chain get the same classes and the same o in mirrored order, an
 * overlapped junction drops the same o bases from either side, and the twin chain's sequence is R(S): strands = 1 still writes
 * exactly one chain of such a pair.
 * Errors.  GK_E_INVALID: the scaffold plan's member and chain errors (an id at or above the bound, or dead; an edge twice; an empty
 * chain; a chain_off that does not ascend), found on the device before a kernel reads a member's length; a parameter out of range;
 * NULL handles or arrays; |G| above 2^31-1 at a junction that is not adjacent.  On any error nothing is written.
 * The defaults the tools and the Python side pass (min_overlap 10, max_overlap k, tol = half the width of the insert range) are
 * choices, not measurements: a chance match of 10 bases has probability 4^-10, about 10^-6, per candidate.
 * On the device: the scaffold plan's check and one lane per junction for last / adjacent / out_of_range; a scan compacts the
 * junctions to search.  k_ovl_search: one wave per junction.  The lanes gather the last min(127, |P(e)|) bases of P(e) and the first
 * min(127, |P(f)|) bases of P(f), two bases per lane and side, and pack them into four 64-bit words per side in LDS (64 bytes per
 * wave).  A lane then takes the candidates lo + lane and lo + lane + 64 (there are at most 127) and tests each by a multi-word
 * shift, mask and compare; a ballot per round counts the hits, and a unique hit is read from the ballot.  No global atomics in the
 * search; the stats are a reduction over jclass and overlap afterwards (one atomic add per wave and counter); one read-back at the
 * end.
 * Not there: overlaps with mismatches or indels, a collective over ranks. */
#define GK_OVERLAP_MAX 127          /* a bound of the implementation, not a measurement */
enum { GK_OVL_LAST = 0, GK_OVL_ADJACENT = 1, GK_OVL_OUT_OF_RANGE = 2, GK_OVL_NONE = 3, GK_OVL_AMBIGUOUS = 4, GK_OVL_OVERLAP = 5 };
int gk_graph_overlap_gaps(gk_graph *g, const uint32_t *members, const uint64_t *chain_off, uint64_t nchains, const int64_t *gap, uint64_t tol,
                          uint32_t min_overlap, uint32_t max_overlap, uint32_t *overlap, uint8_t *jclass, uint64_t *stats7);
/* gk_graph_scaffolds_plan with a third junction class, tested after adjacent:
 *   overlapped  overlap[j] = o > 0 at a junction (members[j], members[j + 1]) that is not adjacent: nothing goes between the
 *               members, and f contributes bases o .. of P(f); its segment row's `skipped` is o.  The gap is not looked at.  Such a
 *               junction counts in neither `gapped` nor `clamped`, and adds nothing to gaps= in the header.
 * `overlap` is parallel to `members` (gk_graph_overlap_gaps' output; the entry at a chain's last member is ignored); NULL, or all
 * zeros, gives gk_graph_scaffolds_plan's text, stats13 and segments bit for bit.  The plan does not trust the array: in the same
 * pass as its other checks, on the device, GK_E_INVALID for an overlap[j] above GK_OVERLAP_MAX, one that is not below both path
 * lengths, a non-zero one at an adjacent junction, or one whose o bases do not match exactly.  So S(c) is always a sequence in
 * which every member's whole path occurs in order, and, a checked overlap being symmetric under twins (above), the strand argument
 * of the scaffold rule carries over unchanged.
 * stats2 = {overlapped junctions, bases dropped (the sum of their o)} over the chain records written. */
int gk_graph_scaffolds_plan_overlaps(gk_graph *g, const uint32_t *members, const uint64_t *chain_off, uint64_t nchains, const int64_t *gap,
                                     const uint32_t *overlap, int64_t min_gap, uint64_t min_len, uint32_t line_width, int strands, int singletons,
                                     gk_scaffolds **out);
int gk_scaffolds_overlap_stats(const gk_scaffolds *s, uint64_t *stats2);
/* live nodes, unspecified order */
int gk_graph_export_nodes(gk_graph *g, uint64_t *lo, uint64_t *hi, uint64_t cap, uint64_t *n);
/* live edges, unspecified order: start/end k-mer, length in bases, and the edge sequence as 2-bit
 * codes packed LSB-first (4 per byte, each edge starting on a byte boundary at seq_off[i]). */
int gk_graph_export_edges(gk_graph *g, uint64_t *start_lo, uint64_t *start_hi, uint64_t *end_lo, uint64_t *end_hi,
                          int64_t *len, int64_t *seq_off, uint64_t cap, uint64_t *n,
                          uint8_t *seq2bit, uint64_t seq_cap, uint64_t *seq_bytes);
/* out-edge insertion order of one node (the reference's immutable Map1..Map4 order, used by
 * removeBubbles); bases4 gets up to 4 base codes, *count their number (-1 = no such node) */
int gk_graph_out_order(gk_graph *g, uint64_t lo, uint64_t hi, int *bases4, int *count);

/* ---- exact two-pass singleton pre-filter -------------------------- */
/* Analogue of the reference's unused Bloom filter (S/ds/BloomFilter.scala:17-70) in front of
 * FreqFilter.add (S/data/FreqFilter.scala:28-36): an array of 2-bit saturating counters, 4 per
 * expected distinct k-mer (1 byte per k-mer instead of a 16/32-byte table slot).
 *   pass 1: gk_prefilter_add_reads[_dev] over EVERY read that will be counted;
 *   pass 2: gk_map_count_reads_prefiltered[_dev] over the same reads: a window enters the table only
 *           if its counter says "seen at least twice".
 * Every k-mer with true count >= 2 then holds its exact count; a k-mer seen once is either absent or
 * present with count 1.  So for rounds >= 2, gk_map_filter_lt(rounds) leaves exactly the table that
 * plain counting + filter_lt(rounds) leaves (FreqFilter.scala:55) — whatever the filter's size. */
int gk_prefilter_create(gk_ctx *ctx, int k, uint64_t expected_distinct, gk_prefilter **out);
void gk_prefilter_destroy(gk_prefilter *pf);
int gk_prefilter_add_reads(gk_prefilter *pf, const uint8_t *bin_host, size_t nbytes, uint64_t nreads);
int gk_prefilter_add_reads_dev(gk_prefilter *pf, const void *dev_records, uint64_t nreads, int read_len);
/* *occurrences = windows looked at, *admitted = windows inserted (either may be NULL).
 * The `_dev` forms take records of one stride, 1 + (read_len + 3) / 4 bytes.  A record whose length byte is below read_len is
 * legal: it contributes its own len - k + 1 windows (none if len < k), and *occurrences and windows_added count those, not
 * nreads x (read_len - k + 1).  A length byte above read_len is GK_E_FORMAT from either `_dev` call (the kernels clamp it, nothing
 * is read past the record); the filter or table may by then hold part of the call's windows, the context stays usable. */
int gk_map_count_reads_prefiltered(gk_map *m, gk_prefilter *pf, const uint8_t *bin_host, size_t nbytes, uint64_t nreads,
                                   uint64_t *occurrences, uint64_t *admitted);
int gk_map_count_reads_prefiltered_dev(gk_map *m, gk_prefilter *pf, const void *dev_records, uint64_t nreads, int read_len,
                                       uint64_t *occurrences, uint64_t *admitted);
/* counters in state "once" / "twice or more", buckets in total, windows fed to pass 1 (any may be NULL) */
int gk_prefilter_stats(gk_prefilter *pf, uint64_t *buckets, uint64_t *seen_once, uint64_t *seen_twice_or_more, uint64_t *windows_added);

/* ---- FASTQ -> `.bin`: Convert2bin (S/scripts/Convert2bin.scala:25-87), parsed on the device ------------------------------
 * The rules (the output is byte-identical to what Convert2bin writes to <out>.bin):
 *   - Lines are Java BufferedReader.readLine lines: a line ends at '\n', at '\r', or at "\r\n" (one terminator, also when it is
 *     split between two pieces of input).  A non-empty unterminated tail at the end of the input is a line; an input that ends
 *     right after a terminator has no further line.
 *   - Records are 4 consecutive lines: header, sequence, separator, quality (:51-73).  Header and separator are not inspected.
 *   - split_at >= 1 (the reference's n = 36): the sequence line and the quality line are each split at split_at characters
 *     (splitAt, :59, :61); a line shorter than that gives an empty second half.  Mate 1 is the first halves, mate 2 the second.
 *     split_at = 0 (interleaved): each record is one whole mate; records 2i and 2i+1 form pair i.
 *   - A mate's length (filtered, :40-49) = min(sequence half's length, quality half's length, index of the half's first
 *     character that is not one of the UPPERCASE A, G, C, T).  'N' and lowercase end a mate; quality values are otherwise ignored.
 *   - Output per mate: [len:u8] then ceil(len/4) bytes of 2-bit codes A0 G1 C2 T3 packed LSB-first (:35-38); mate 1 before
 *     mate 2, one pair per record (per two records, interleaved).
 *   - Statistics (:32-47, :85-87): pairs = pairs emitted; kmers = sum of len - k_stats + 1 over the mates with len >= k_stats
 *     (the reference's k = 23); short_pairs = pairs with a mate shorter than k_stats.
 *   - End of input: a trailing lone header line is ignored (Convert2bin stops when the sequence readLine returns null); a
 *     trailing record of 2 or 3 lines is GK_E_FORMAT (the reference crashes on the null quality line).
 * Deliberate deviations from the reference, each GK_E_FORMAT instead of silent garbage: a mate longer than 255 (the reference
 * writes length.toByte, which wraps); a byte >= 0x80 in a sequence or quality line (the reference splits at characters of the
 * platform charset; this converter is ASCII only); a single record of more than 64 MiB of text; an odd number of records at the
 * end of interleaved input.  Every such message names the 0-based record number ("FASTQ record N: ...", gk_last_error).
 * The PairedEndData descriptor (:83) is not written: the pair count is reported (gk_fastq_stats) and the tools take it. */
/* split_at >= 1: Convert2bin's n; 0: interleaved.  k_stats in 1..255 (the `kmers` / `short_pairs` statistics).
 * max_pairs: stop emitting after that many pairs (0 = all; later records are still parsed for errors and counted as text
 * only) - GraphBuilder's genome.takeFirst.  Device memory comes from the context's block pool (gk_ctx_mem_stats) and is released
 * by gk_fastq_destroy. */
int gk_fastq_create(gk_ctx *ctx, int split_at, int k_stats, uint64_t max_pairs, gk_fastq **out);
void gk_fastq_destroy(gk_fastq *fq);
/* Parse the next piece of text (last != 0: the input ends with it; later calls are GK_E_STATE).  An incomplete trailing record
 * is kept in the handle ("carried") and completed by the next call.  Appends the .bin records of every completed pair to
 * bin_out, *bin_bytes = bytes appended.  `text` may be pageable or pinned (gk_host_alloc / gk_host_register; pageable text is
 * staged through pinned buffers).  Long calls are cut into device chunks; the next chunk's upload runs on the context's copy
 * stream beside this chunk's kernels.
 * BOUND: what one call writes never exceeds (bytes carried in) + nbytes, so a bin_cap below that is GK_E_CAPACITY before
 * anything is consumed (the handle is unchanged: retry with a larger buffer).  Proof: the records a call completes lie in the
 * carried bytes and the new text, and no two overlap.  A completed record has at least 3 terminator bytes (its header, sequence
 * and separator lines are followed by a line) besides its sequence line of S characters.  Its mates have lengths l1 + l2 <= S
 * (l1 <= the first half, l2 <= the second half; one mate of l <= S when interleaved), and a mate writes 1 + ceil(l/4) <= 1 + l
 * bytes: at most 2 + S < S + 3 bytes per record.
 * After any other error the handle refuses further calls with GK_E_STATE; after GK_E_FORMAT bin_out holds every pair before
 * the bad record and nothing past the last good pair (*bin_bytes says how much). */
int gk_fastq_convert(gk_fastq *fq, const char *text, size_t nbytes, int last, uint8_t *bin_out, size_t bin_cap, size_t *bin_bytes);
/* The same parse, but the mates are counted into m (k = gk_map_k(m), same context) straight from device memory (FreqFilter.add,
 * as gk_map_count_reads), with no .bin crossing to the host.  The table afterwards equals, bit for bit, the one
 * gk_map_count_reads of the converted stream gives; *occurrences = windows counted by this call.  Inserts are cut into batches
 * of at most the map's window limit from a device prefix sum of windows per mate.  On an error the promise is
 * gk_map_count_reads' for a truncated stream: the pairs before the bad record, or chunks of them, may already be counted. */
int gk_fastq_count(gk_fastq *fq, gk_map *m, const char *text, size_t nbytes, int last, uint64_t *occurrences);
/* pairs, short_pairs, kmers (so far), text bytes consumed, bytes carried now (any may be NULL).  The carried count is what lets a
 * caller size the next bin_out: carried + nbytes. */
int gk_fastq_stats(const gk_fastq *fq, uint64_t *pairs, uint64_t *short_pairs, uint64_t *kmers, uint64_t *text_bytes,
                   uint64_t *carried_bytes);
/* wall ms of the last call: {host staging + upload, parse kernels, download or count, whole call} */
int gk_fastq_last_ms(const gk_fastq *fq, float *ms4);

/* ---- FASTA check: the k-window loop of CheckGraph (S/scripts/CheckGraph.scala:48-55), on the device ----------------------
 * Every k-window of a reference FASTA is looked up in a position map (normally gk_graph_position_map of the graph under test);
 * k = gk_vmap_k of that map.  The text is fed in pieces of any size, as for the FASTQ parser.  The rules:
 *   - Lines are readLine lines exactly as in the FASTQ section: a line ends at '\n', at '\r', or at "\r\n" (one terminator, also
 *     when it is split between two feeds).  A non-empty unterminated tail at the end of the input is a line.  `lines` counts them.
 *   - A line whose first character is '>' is a header (:48).  A header starts a new record; sequence lines before the first
 *     header belong to record 0.  `records` = headers, plus one if a sequence character precedes the first header.
 *   - Every character of every other line is a sequence character (`bases`).  It is valid only if it is an UPPERCASE A, G, C or T
 *     (Base.fromChar, :49; `valid_bases`).  'N', lowercase and bytes >= 0x80 are invalid; they are not an error.
 *   - A window is k consecutive sequence characters, all valid, inside one line (per_line != 0: the reference's literal rule,
 *     line.sliding(k)) or inside one record (per_line == 0: the record's sequence lines are joined, so windows cross line ends
 *     but never a header).  `windows` counts them.  A window is looked up as it reads, not canonicalised (getGraphMap stores
 *     node.seq and the k-mers along every edge as they are, and the graph holds both strands).  The lookup is `contains` (:51):
 *     the first slot of the probe sequence that holds the key, as gk_vmap_get_batch.  found + missing == windows.
 *   - `covered_bases` = sequence characters that lie inside at least one found window.  covered_bases / valid_bases is the
 *     "coverage" figure quoted for the reference.
 *   - `short_lines` = non-header lines of 1..k-1 characters.  DEVIATION: the reference's sliding(k) yields such a line whole and
 *     logs it as "Not found"; here it has no window (in either mode's own terms) and is counted in short_lines, whatever its
 *     characters.
 *   - The missing list holds the first max_missing not-found windows in stream order (an ordered compaction: the same list on
 *     every run and for every way of cutting the input into feeds).  Each entry: the byte offset of the window's first base in
 *     the whole input, that base's 0-based line and 0-based column, and the k-mer (base i at bits 2i of lo, then hi).
 *     DEVIATION: the reference logs line.length; a line can outlast a feed, so line and column are reported instead.
 *   - No text is kept between feeds (an unwrapped chromosome on one line needs no buffering): the handle carries the last k-1
 *     sequence codes and the line state.  Long feeds are cut into device slices; the next slice's upload runs on the context's
 *     copy stream beside the current slice's kernels.
 * Errors: a null handle is GK_E_INVALID; a feed after last != 0 is GK_E_STATE; after any other error the handle refuses further
 * feeds with GK_E_STATE.  Device memory comes from the context's block pool (gk_ctx_mem_stats): each feed's buffers are returned
 * when the feed returns, the rest by gk_fasta_check_destroy.  The position map must outlive the handle and not change under it. */
typedef struct gk_fasta_check gk_fasta_check;
/* positions: any gk_vmap of this context.  max_missing: how many not-found windows to keep (0 = none). */
int gk_fasta_check_create(gk_ctx *ctx, gk_vmap *positions, int per_line, uint64_t max_missing, gk_fasta_check **out);
void gk_fasta_check_destroy(gk_fasta_check *fc);
/* the next piece of text (pageable or pinned); last != 0: the input ends with it */
int gk_fasta_check_feed(gk_fasta_check *fc, const char *text, size_t nbytes, int last);
/* the counters so far (any may be NULL).  Windows that start in the last k-1 sequence characters fed so far are evaluated by
 * the next feed, and an unterminated last line is counted when the input ends: the figures are final after last != 0. */
int gk_fasta_check_stats(const gk_fasta_check *fc, uint64_t *lines, uint64_t *records, uint64_t *bases, uint64_t *valid_bases,
                         uint64_t *windows, uint64_t *found, uint64_t *missing, uint64_t *covered_bases, uint64_t *short_lines);
/* the missing list: *n = entries held (<= max_missing); the first min(*n, cap) are written (any array may be NULL) */
int gk_fasta_check_missing(const gk_fasta_check *fc, uint64_t *text_offset, uint64_t *line, uint64_t *column,
                           uint64_t *lo, uint64_t *hi, uint64_t cap, uint64_t *n);
/* wall ms of the last feed: {host staging + upload, parse kernels, lookup kernels, whole call} */
int gk_fasta_check_last_ms(const gk_fasta_check *fc, float *ms4);

/* ---- placements: this project's own rule (the reference's CheckGraph asks whether a window of the genome is in the graph, never
 * where an edge lies) ----
 * Every edge of a graph placed on a reference genome: for each edge and strand, how many windows of the reference hit it and on
 * which diagonal.  Integers only.
 * Input.  One reference record per gk_placements_add_record call, as its joined sequence characters: the caller splits the FASTA
 * text by the record rule of the "FASTA check" section with per_line == 0 (headers start records, sequence lines before the first
 * header are record 0, terminators are dropped).  Records are numbered 0, 1, ... in call order.  A character is valid iff it is an
 * UPPERCASE A, G, C or T; a window is k consecutive valid characters of one record, k = gk_vmap_k of the position map.  Long
 * records are cut into device slices; a slice brings the k-1 characters before it along, so nothing is carried between slices, and
 * the next slice's upload runs on the context's copy stream beside the current slice's kernel.
 * Lookups.  P(e) = start k-mer ++ seq is the path of edge e, as in the contig rule.  For the window W at record coordinate x
 * (0-based, of its first character) BOTH W and revComplement(W) are looked up as they read, with getAll and the position decoding
 * of gk_graph_pair_links.  Each of the two lookups falls into exactly one class, tested in this order:
 *   absent      the list is empty;
 *   repetitive  the list has two or more entries: they are not looked at;
 *   at_node     the single position is a NODE position;
 *   edge        the single position is Edge(e, d), 1 <= d <= len_e - 1.
 * Candidates.  An `edge` hit of W at Edge(e, d) gives the FORWARD candidate (r, x - d) for e: the record coordinate of base 0 of
 * P(e), with P(e) reading toward higher coordinates.  An `edge` hit of revComplement(W) at Edge(e', d') gives the REVERSE candidate
 * (r, x + d' + k - 1) for e': the record coordinate of base 0 of P(e'), with P(e') reading toward lower coordinates (the window's
 * last character, at x + k - 1, is the complement of base d' of P(e'), and base 0 lies d' characters further up).
 * Both are constant along a diagonal: if the reference spells P(e) forward from coordinate c, the window at x = c + d is the k-mer
 * at distance d, so x - d = c for every d; if it spells the reverse complement of P(e) ending at coordinate c, the window at x is
 * the reverse complement of the k-mer at distance d = c - (x + k - 1), so x + d + k - 1 = c for every d.
 * Per edge and strand the table holds a u32 hit count and the minimum and maximum of the candidate packed as
 * record << 40 | (coordinate + 2^39).  More than 2^24 records, or a record of 2^39 bases or more, is GK_E_CAPACITY.  A count that
 * would pass 2^32-1 saturates at 2^32-1 (no test reaches this: it takes 2^32 hits of one edge).
 * Edge classes: the first that holds (gk_placements_edges' cls):
 *   0 unplaced      no hit on either strand (a live edge with len == 1 has no interior k-mer and is always unplaced);
 *   1 both_strands  hits on both strands;
 *   2 scattered     min != max on the hit strand: a repeat, or an edge that differs from the reference by an indel;
 *   3 forward, 4 reverse   exactly one diagonal; `record` and `pos` (the candidate's coordinate, which may be negative or lie past
 *                   the record's end when the reference covers only part of P(e)) are set, and are 0 in every other class.
 * windows_fwd / windows_rev are the two hit counts.  A dead edge id gives unplaced and zeros.  An id at or above the bound the
 * graph had at create is GK_E_INVALID with nothing written.  Any output array may be NULL.
 * Stats: uint64[GK_PLACE_NSTATS] = {records, bases, valid_bases, windows, fwd absent, fwd repetitive, fwd at_node, fwd edge, rev
 * absent, rev repetitive, rev at_node, rev edge, edges unplaced, both_strands, scattered, forward, reverse, path bases (k + len)
 * of the forward edges, of the reverse edges, edges with a saturated count}.  Identities: [4] + [5] + [6] + [7] = [3] and
 * [8] + [9] + [10] + [11] = [3]; [12] + .. + [16] = the live edges; [2] <= [1]; [19] counts live edges only.
 * Errors.  gk_placements_create: GK_E_KLEN for a position map of another k, GK_E_INVALID for NULL handles or a map of another
 * context.  gk_placements_add_record: GK_E_STATE for a stale position map (a position that names nothing live in this graph:
 * tested, bound first, before any per-edge array is indexed by it); after a failed add_record the handle refuses further records
 * with GK_E_STATE.  Every call but destroy and last_ms returns GK_E_STATE once the graph has been edited since create.  Device
 * memory comes from the context's block pool; a call's slice buffers go back when it returns.  The graph and the position map must
 * outlive the handle; neither is changed.
 * On the device: a lane owns 16 consecutive window starts of the slice, staged in LDS with a k-1 halo, and rolls W and its
 * reverse complement together; hits of one edge are folded to (count, min, max) inside the lane's run and again over the wave, and
 * one 32-bit add plus a 64-bit min and a 64-bit max go to HBM per folded run.
 * Not there: a collective over ranks, circular references.  Alignment inside a scattered edge is the next section's. */
#define GK_PLACE_NSTATS 20
enum { GK_PLACE_UNPLACED = 0, GK_PLACE_BOTH_STRANDS = 1, GK_PLACE_SCATTERED = 2, GK_PLACE_FORWARD = 3, GK_PLACE_REVERSE = 4 };
typedef struct gk_placements gk_placements;
int gk_placements_create(gk_graph *g, gk_vmap *positions, gk_placements **out);
void gk_placements_destroy(gk_placements *p);
int gk_placements_add_record(gk_placements *p, const char *bases, uint64_t n);
int gk_placements_stats(const gk_placements *p, uint64_t *stats);
int gk_placements_edges(const gk_placements *p, const uint32_t *edge_ids, uint64_t n, uint8_t *cls, uint32_t *record, int64_t *pos,
                        uint32_t *windows_fwd, uint32_t *windows_rev);
/* wall ms of the last add_record: {host staging + upload, 0, lookup kernels, whole call} */
int gk_placements_last_ms(const gk_placements *p, float *ms4);

/* ---- the judge: every junction of a scaffold plan against the placements.  This project's own rule. ----
 * A written piece of a plan is always bases skipped .. of P(edge) read FORWARD, whichever strand the chain was selected on
 * (`strands` only selects which chains are written, gk_scaffolds.hip), so one rule serves strands = 1 and 2.
 * A junction is two consecutive rows of gk_scaffolds_segments with the same `record`; the outputs are parallel to those rows in
 * row order: *n = rows - records.  Its KIND is what the plan recorded: gapped (1) iff an N run lies between the two rows; else
 * adjacent (0) iff the first row's edge ends at the node ID the second row's edge starts at; else overlapped (2).  That IS the plan's
 * own class of the junction, read back from what it wrote: the plan tests `adjacent` first and by the same node IDs, min_gap >= 1
 * makes every gapped junction write an N run, and an overlapped one writes none (skipped alone cannot tell an overlap of exactly k
 * bases from an adjacent junction, so the node IDs decide it, as in the plan).
 * Distances.  Rows (e, first_e, skipped_e) and (f, first_f, skipped_f): dscaf = first_f - first_e; with both edges forward
 * dref = (pos_f + skipped_f) - (pos_e + skipped_e); with both reverse dref = (pos_e - skipped_e) - (pos_f - skipped_f);
 * err = dscaf - dref.
 * Classes, tested in this order:
 *   0 unjudged      either edge is not placed forward or reverse;
 *   1 other_record  the two edges are placed on different reference records;
 *   2 strand        one edge is forward and the other reverse;
 *   3 order         dref <= 0;
 *   4 distance      |err| > tol at a gapped junction, err != 0 at an adjacent or overlapped one (those write no N and must fit);
 *   5 correct       none of the above.
 * err[j] is written for order, distance and correct, and is 0 otherwise.  A MISJOIN is a junction of class 1 .. 4.
 * Stats: uint64[GK_JUDGE_NSTATS] = {junctions, the six classes [1 + c], the six classes of the adjacent junctions [7 + c], of the
 * gapped [13 + c], of the overlapped [19 + c], [25] the sum and [26] the maximum of |err| over the correct gapped junctions, [27]
 * chain records with at least one junction that is not unjudged, [28] chain records with no misjoin}.  Identities: [1] + .. + [6]
 * = [0]; [1 + c] = [7 + c] + [13 + c] + [19 + c]; [27], [28] <= the plan's chain records; a chain record without junctions has no
 * misjoin.
 * Known limit: a join across the two ends of a circular chromosome is classed `order`; there is no circular mode.
 * tol has no measured value: the tools' --judge-tol defaults to their fill / overlap TOL, half the width of the insert range, as a
 * choice.
 * Errors: GK_E_INVALID for NULL handles, or a plan and placements of different graphs or contexts; GK_E_STATE if the graph was
 * edited; cap below *n is GK_E_CAPACITY with *n and the stats set and nothing copied.
 * On the device: one lane per segment of the plan, the junction's index from a scan over the edge segments; the stats by ballot
 * and one atomic per wave. */
#define GK_JUDGE_NSTATS 29
enum { GK_JUDGE_UNJUDGED = 0, GK_JUDGE_OTHER_RECORD = 1, GK_JUDGE_STRAND = 2, GK_JUDGE_ORDER = 3, GK_JUDGE_DISTANCE = 4, GK_JUDGE_CORRECT = 5 };
int gk_scaffolds_judge(const gk_scaffolds *s, const gk_placements *p, uint64_t tol, uint8_t *cls, int64_t *err, uint64_t cap, uint64_t *n,
                       uint64_t *stats);

/* ---- alignment blocks: this project's own rule (the placements fold the hits of an edge to one count, one minimum and one
 * maximum; this pass keeps the runs) ----
 * Every edge of a graph aligned to a reference genome as the exact runs of k-mers it shares with it.  Integers only.
 * Hits.  The input, the validity of characters, the windows, the two lookups per window and the candidates are exactly those of
 * "placements".  For strand s (0: W as it reads, 1: revComplement(W)) and window start x of record r the HIT h_s(x) is (e, c) when
 * the lookup's class is `edge`: e the edge, c the candidate, x - d for a forward hit and x + d + k - 1 for a reverse hit.  It is
 * NONE otherwise: absent, repetitive, at_node, and no valid window at x.
 * Run.  A run is a maximal interval x0 .. x1 of consecutive window starts of one record and one strand with the same hit that is
 * not NONE.  Equal (e, c) at consecutive x means consecutive d, so a run is an exact match of n = x1 - x0 + 1 consecutive k-mers
 * of P(e).
 * Block row.  (edge, strand, record, pos = c, dlo, dhi); dlo .. dhi is the inclusive range of k-mer distances of the run:
 * forward dlo = x0 - c, dhi = x1 - c; reverse dlo = c - (x1 + k - 1), dhi = c - (x0 + k - 1).  1 <= dlo <= dhi <= len_e - 1.
 * Order.  Rows are ordered by (edge, dlo, dhi, strand, record, x0).  Two rows of one strand and record differ in x0, so the order
 * is total; rows are numbered in it, and an edge's rows are consecutive.
 *
 * ---- breakpoints ----
 * Every row after the first row of its edge carries a breakpoint class against the row before it, the first that holds:
 *   1 overlap        dlo <= dhi of the row before: the same graph k-mer lies at two places of the reference;
 *   2 translocation  another record;
 *   3 inversion      another strand;
 *   4 relocation     |shift| > tol;
 *   5 indel          0 < |shift| <= tol;
 *   6 colinear       shift == 0: substitutions, N or lowercase in between.
 * The first row of an edge has class 0.  shift of rows i, i + 1 (same record and strand) = pos(i + 1) - pos(i) when forward and
 * pos(i) - pos(i + 1) when reverse: positive means the reference holds that many more bases between the two blocks than P(e)
 * does.  `shift` is written per row and is 0 for the classes 0 to 3.
 * Adjacent rows are enough for `overlap`: if rows i < j of an edge overlap, dlo(j) <= dhi(i), then the order gives
 * dlo(i) <= dlo(i + 1) <= dlo(j) <= dhi(i), so row i + 1 overlaps row i already: an edge has some overlapping pair of rows iff it
 * has an `overlap` breakpoint.
 * Edge classes, the first that holds (gk_blocks_edges' cls):
 *   0 unaligned     no row;
 *   1 repeat        some `overlap` breakpoint;
 *   2 misassembled  some breakpoint of class 2 to 4;
 *   3 indel         some breakpoint of class 5;
 *   4 colinear      more than one row, all breakpoints of class 6;
 *   5 exact         one row.
 * `full` is set iff the edge's first row has dlo == 1 and its last row has dhi == len_e - 1.  first_row and nrows give the edge's
 * rows by number.  A dead edge id gives unaligned and zeros; an id at or above the bound the graph had at create is
 * GK_E_INVALID with nothing written.
 * Pieces.  For every edge that is not `repeat` the row list is cut at every breakpoint of class 2 to 4; a piece spans
 * (dhi of its last row - dlo of its first row + k) bases.  gk_blocks_pieces gives (bases, edge) in row order.  NA50 and NGA50 are
 * the caller's to compute from the piece lengths, as from gk_scaffolds_segments' rows: lengths descending, the first at which
 * twice the running sum reaches the piece bases [21] (NA50) or the valid bases of the reference [2] (NGA50; 0 if never).
 * Stats: uint64[GK_BLOCKS_NSTATS] = {records, bases, valid_bases, windows, [4] covered: windows with an `edge` hit on at least
 * one strand (the numerator of the genome fraction, over [3]), [5] rows, [6 .. 11] the breakpoint classes 1 .. 6, [12 .. 17] the
 * edge classes 0 .. 5, [18] full edges, [19] aligned k-mers: the sum of n over all rows, [20] pieces, [21] piece bases, [22] the
 * sum and [23] the maximum of |shift| over the `indel` breakpoints}.  Identities: [12] + .. + [17] = the live edges;
 * [6] + .. + [11] = [5] - ([13] + .. + [17]) (every aligned edge has one first row); [2] <= [1]; [4] <= [3]; [4] <= [19] <= 2 [3];
 * [20] >= [14] + .. + [17]; [18] <= [13] + .. + [17]; [23] <= [22].
 * Strand symmetry.  Where the graph holds both e and its twin e' (P(e') = revComplement(P(e)), len the same), the k-mer at
 * distance d of P(e') is the reverse complement of the k-mer at distance len - d of P(e).  So W hits Edge(e, d) iff
 * revComplement(W) hits Edge(e', len - d): every forward run of e is a reverse run of e' over the same starts and the other way
 * round, with d -> len - d, hence (dlo, dhi) -> (len - dhi, len - dlo), and pos' = pos + len + k - 1 for a forward row of e,
 * pos' = pos - len - k + 1 for a reverse one.  The map d -> len - d reverses the order of an edge's rows wherever the order is
 * decided by non-overlapping ranges, so neighbours stay neighbours: records agree, strands are flipped on both sides of a
 * breakpoint, and pos(i + 1) - pos(i) of a forward pair becomes pos'(i) - pos'(i + 1) of the reverse pair read the other way
 * round: the classes and |shift| agree (the sign of shift too).  An overlap stays an overlap.  Both edge classes and `full`
 * agree; within a repeat the order of overlapping rows, and with it the sequence of their classes, may differ.
 * Limits.  tol is a choice, not a measurement: the tools' --block-tol defaults to 1000.  The capacity rules are the placements'
 * own (2^24 records, records below 2^39 bases: GK_E_CAPACITY); more than 2^32 - 1 rows is GK_E_CAPACITY from gk_blocks_finish.
 * Calls.  gk_blocks_add_record feeds one record, as gk_placements_add_record does (slices of the record honour the same test
 * switch; a slice brings k characters along, one more than the placements', for the hit before its first start).
 * gk_blocks_finish(tol) orders the rows, classes every breakpoint and edge and cuts the pieces; it may be called again with
 * another tol, without feeding the records again.  gk_blocks_rows: any array may be NULL; cap below *n is GK_E_CAPACITY with *n
 * set and nothing copied (so does gk_blocks_pieces).
 * Errors are the placements' own (GK_E_KLEN, GK_E_INVALID, GK_E_STATE for a stale position map, tested bound first before any
 * per-edge array is indexed, and for an edited graph).  In addition: stats, rows, edges and pieces before the first finish are
 * GK_E_STATE, and so is add_record after a finish.
 * On the device: gk_blocks.hip.  A window start is an EVENT on a strand iff its hit differs from the hit one start before (NONE
 * before a record's first window; a change to NONE is an event too), a definition that knows nothing of lanes, waves, tiles or
 * slices.  A run is an event with a hit; it ends one start before the next event of its strand.  A count launch, a scan over
 * the workgroups' counts and an emit launch write the events in stream order with plain 16-byte stores; every window is looked
 * up twice, which is accepted for an instrument.  The event buffers come from the context's block pool and grow between slices.
 * Not there: a collective over ranks, circular references, any alignment with mismatches inside a block, feeding the result
 * back into gk_scaffolds_judge (whose classes do not change). */
#define GK_BLOCKS_NSTATS 24
enum { GK_BREAK_FIRST = 0, GK_BREAK_OVERLAP = 1, GK_BREAK_TRANSLOCATION = 2, GK_BREAK_INVERSION = 3, GK_BREAK_RELOCATION = 4, GK_BREAK_INDEL = 5,
       GK_BREAK_COLINEAR = 6 };
enum { GK_BLOCKS_UNALIGNED = 0, GK_BLOCKS_REPEAT = 1, GK_BLOCKS_MISASSEMBLED = 2, GK_BLOCKS_INDEL = 3, GK_BLOCKS_COLINEAR = 4, GK_BLOCKS_EXACT = 5 };
typedef struct gk_blocks gk_blocks;
int gk_blocks_create(gk_graph *g, gk_vmap *positions, gk_blocks **out);
void gk_blocks_destroy(gk_blocks *b);
int gk_blocks_add_record(gk_blocks *b, const char *bases, uint64_t n);
int gk_blocks_finish(gk_blocks *b, uint64_t tol);
int gk_blocks_stats(const gk_blocks *b, uint64_t *stats);
int gk_blocks_rows(const gk_blocks *b, uint32_t *edge, uint8_t *strand, uint32_t *record, int64_t *pos, uint32_t *dlo, uint32_t *dhi, uint8_t *brk,
                   int64_t *shift, uint64_t cap, uint64_t *n);
int gk_blocks_edges(const gk_blocks *b, const uint32_t *edge_ids, uint64_t n, uint8_t *cls, uint8_t *full, uint32_t *first_row, uint32_t *nrows);
int gk_blocks_pieces(const gk_blocks *b, uint64_t *len, uint32_t *edge, uint64_t cap, uint64_t *n);
/* wall ms: {host staging + upload, count launches + scans, emit launches, whole call} of the last add_record, {device time, whole
 * call} of the last finish */
int gk_blocks_last_ms(const gk_blocks *b, float *ms6);

/* ---- synthetic reads (bench / tests) ---------------------------------------- */
/* Fill dev_records with nreads fixed-length `.bin` records generated on device, bit-identical to
 * genome_amd/synth.py.  mode 0 = U (uniform bases); mode 1 = G (genome of G bases, error rate
 * err_thresh24 / 2^24).  first_read offsets the stream so chunks can be generated independently. */
int gk_synth_reads_dev(gk_ctx *ctx, void *dev_records, uint64_t nreads, int read_len, int mode, uint64_t config_id,
                       uint64_t first_read, uint64_t genome_len, uint32_t err_thresh24);

#ifdef __cplusplus
}
#endif
#endif

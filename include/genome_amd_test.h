/*
 * genome_amd_test.h — entry points that exist ONLY in the test build of the library (genome_amd/libgenome_amd_test.so =
 * libgenome_amd.so's objects + csrc/gk_testhooks.o).  The product library exports none of them, reads no environment variable
 * and has no switch a host could flip by accident.  tests/conftest.py points the Python binding at the test build
 * (GK_LIB_PATH); the kernels, the C-ABI of include/genome_amd.h and everything behind it are the same objects in both.
 */
#ifndef GENOME_AMD_TEST_H
#define GENOME_AMD_TEST_H

#include "genome_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test / A-B switches.  Their defaults are read from the environment ONCE, in
 * gk_ctx_create (GK_TEST_NO_RESERVE, GK_HOST_RAGGED, GK_PART_EXACT, GK_GRAPH_UNITIGS=walk|pj); no entry point
 * consults the environment afterwards.  Names: "test_no_reserve", "host_ragged", "part_exact" (0/1),
 * "graph_unitigs" (0 auto, 1 walk, 2 pointer jumping), "graph_walk_queue" (0: one edge per lane), "graph_load_pct" (load factor
 * of the compacted table, percent), "p4_direct" / "fine_exact" / "p2_wide" / "p2_sorted" (-1 auto, 0, 1), "p4_wide" (-1 auto, 0: 4096-key sorts, 1: 8192, 2: 12288),
 * "p45_stripes" (P5 of one stripe of L1 buckets beside P4 of the next), "p24_pieces" (P4 of one piece of a batch beside the L1
 * scatter of the next), "p4_grid" (P4 workgroups per CU), "filter_classic" (1: tombstones + rehash instead of the streaming
 * rebuild), "dist_exchange_ahead" (0: gk_dist_count_routed does not post the next batch's exchange ahead; every rank alike):
 * A/B switches of the kernels in gk_partition.hip / gk_graph.hip / gk_dist.hip; what each measured is in DESIGN.md and
 * profiles/r02.  "min_lnb1" (also GK_MIN_LNB1; 9 / 10: tables of enough segments get 512 / 1024 L1 buckets, the fan-out of
 * tables beyond 34 GB) and "test_max_nb2" (the pipeline refuses tables of more fine buckets per L1 bucket) stage the
 * large-table paths on small tables.
 * Round 3: "graph_mbt" / "graph_mbt_keys" (gk_graph_build on a minimizer-bucketed copy of the table; keys per bucket),
 * "pairs_host" (1: the paired-end walks on host threads), "thread_combine" (1: gk_graph_thread_reads combines the equal keys of
 * a wave's trip before the atomic instead of adding every crossing with an atomic of its own), "test_pairs_small_sets" (tiny LDS sets: walks overflow to the host
 * walker), "host_prefetch" (0: a host-fed count does not upload the next chunk beside the current one), "test_max_stage" (bytes
 * per staging area of a host-fed count), "cc_find" (the components' link pass: 3 = look before the CAS, the default; 0 / 1 / 2 =
 * path halving only / no path writes / start node only), "target_load_pct" (load factor new tables are sized for, percent;
 * 0 or -1 = the default, 65; else 10..75, anything else is GK_E_INVALID: the growth limit is 80 and a table sized for a load at or
 * above it grows for ever or fills a segment; ignored at k = 64, whose tagged table is always sized for 45), "graph_load_pct" (the
 * same range and refusal; 0 or -1 = chosen by free memory; at k = 64 a value above 45 means 45, the tagged table's densest step),
 * and the failure injections of the exchange: "test_dist_small_send" (a send region far too small: re-routed in place), "test_dist_fail_exchange" (this rank's next exchange fails locally with the given code), "test_dist_fail_classify"
 * (this rank cannot stage the queries of its next classified gather), "test_dist_fail_reduce" (this rank fails the owner merge of
 * its next gk_dist_reduce_support, gk_dist_reduce_links or gk_dist_reduce_spans, after the records were exchanged).
 * "test_max_grid" (0: off; a positive value: every grid-stride launch of the graph phase — build, simplify, components,
 * coverage, tips, bubbles, distance, export, the graph file, the position map, the paired-end stage —, of the value maps, the
 * spectrum and the read correction gets at most that many workgroups, the pair walks twice as many, instead of 8 (16) per CU; a
 * negative value is GK_E_INVALID): a graph the oracle can follow then makes every workgroup take several trips through its loop,
 * and one workgroup sees more component roots than its LDS table holds.  The insert pipeline's grids follow the table's geometry
 * and are not capped; gk_map_verify's one pass over the slots is (its checksum is what the tests compare tables by).  The owner
 * routing is capped as well: the one launch of gk_shard_superkmers_dev (and of the routing inside gk_dist_*, fixed stride or
 * offset table: 6 workgroups per CU when the switch is 0) and both launches of gk_shard_reads_dev, so that 200 reads — four
 * tiles — make one workgroup take a regrouped tile and then ordinary ones and carry its counters across tiles.  The list of capped kernels is in DESIGN.md section 5.  The contig kernels (gk_graph_contigs_plan,
 * gk_contigs_read / gk_contigs_write) are capped by it too.
 * "contigs_chunk_bytes" (0: the default, 64 MiB; else rounded down to a multiple of 8, at least 8): the bytes of FASTA text
 * gk_contigs_read / gk_contigs_write emit per device chunk, so that a text of a few KiB goes through many chunks and both
 * staging buffers.
 * "twin_key_bits" (0..128, the default and the product: 128; anything else is GK_E_INVALID): both content keys of
 * gk_graph_edge_twins / gk_graph_gfa_plan are cut to their low bits.  With few bits a run of equal keys holds many edges of
 * different content, so the exact confirmation and the walk along a run decide every answer; at 0 every live edge is in one run
 * (quadratic: for graphs of a few hundred edges).  The answers do not change, only `key_collisions`.  The GFA text's chunks follow
 * "contigs_chunk_bytes" and the twin and GFA kernels' grids "test_max_grid".
 * "test_place_slice" (0: the default, 64 Mi characters): the characters of a reference record gk_placements_add_record puts
 * through the device per slice, so that a record of a few kbp is cut inside a contig and both upload buffers are used.
 * The singleton pre-filter: "test_max_stage" is also the bytes of `.bin` records its host-fed passes stage per chunk (0: 256 MiB),
 * "test_prefilter_chunk_windows" (0: the default, 2^28) the k-mer windows of one pass-2 chunk, of the host-fed call and of the
 * `_dev` call alike, and its three launches (both passes and the counters' census of gk_prefilter_stats) obey "test_max_grid".
 * "test_multik_chunk_windows" (0: the default, 2^24): the k-mer windows of one chunk of gk_map_add_graph_paths, rounded down to
 * whole runs of 16 windows and at least one run, so that a graph of a few thousand windows goes through many chunks; its
 * classification and emission launches obey "test_max_grid". */
int gk_ctx_set_option(gk_ctx *ctx, const char *name, int64_t value);

/* The echo of the pre-filter's chunking: what this filter handle has run since it was created.  *host_fixed / *host_offsets = the
 * chunks its host-fed calls (either pass) staged as a run of equal-length records with a fixed stride / with an offset table;
 * *dev_pass2 = the chunks of gk_map_count_reads_prefiltered_dev; *pass2_launches = launches of the pass-2 kernel (a staged chunk
 * without a window launches none).  Any pointer may be null; a null handle is GK_E_INVALID. */
int gk_test_prefilter_chunks(const gk_prefilter *pf, uint64_t *host_fixed, uint64_t *host_offsets, uint64_t *dev_pass2, uint64_t *pass2_launches);

/* The echo of "test_multik_chunk_windows": *chunks = the chunks the last gk_map_add_graph_paths on this context emitted and
 * inserted (0 after a call that was refused or found no window). */
int gk_test_multik_chunks(const gk_ctx *ctx, uint64_t *chunks);

/* The echo of "test_max_grid": *uses = the launches on this context whose grid was bounded by the switch's value instead of by
 * 8 workgroups per CU, since the context was created (every capped launch site asks once per launch; nothing is counted while the
 * switch is 0).  A call that is meant to run under the cap and leaves the number as it was did not consult it. */
int gk_test_grid_cap_uses(const gk_ctx *ctx, uint64_t *uses);

/* What one batch of the partitioned insert would choose (gk_partition.hip: part_choose, the function part_run takes every choice
 * from), for plain values instead of a context and a map: no device is touched, and the call works on a machine without one.  So
 * the auto rules of tables far too large for a test — which member of P4's family from how many fine buckets per L1 bucket, and
 * what still fits the CU's LDS — are held to literals by tests/test_part_plan_cpu.py.
 * in: W (1 / 2 key words), lnb1 (0..10) and nb2 (the table's geometry); source (0 device records of one length, 1 the same in
 * host memory, 2 the same prefetched, 3 a ragged stream, 4 keys) and max_windows (windows of the longest record; 0 for ragged
 * streams and keys); from_empty, estimate and fine_exact (PartPlan's: the "fine_exact" switch arrives through it),
 * verify_uniform; the switches "part_exact", "p4_wide", "p4_direct", "p2_wide", "p2_sorted", "p45_stripes", "p24_pieces", "p4_grid"
 * and "test_max_nb2" as gk_ctx_set_option takes them (-1 auto; 0 for the two test switches).
 * out: P4's member on the over-provisioned and on the exact fine level — its "last_p4" name, keys per chunk, threads, dynamic
 * LDS bytes for this geometry —, the "last_p2" name, part_supported, the batch's first choices (op1, fine_exact — which the
 * sample may revise between the levels —, sync_between, pipelined) and the stripes of the level it starts with (1 when exact).
 * GK_E_INVALID for a null pointer, W, lnb1 or source out of range. */
typedef struct gk_test_part_in {
    int32_t W, lnb1;
    uint32_t nb2;
    int32_t source, max_windows, from_empty, estimate, fine_exact, verify_uniform;
    int32_t part_exact, p4_wide, p4_direct, p2_wide, p2_sorted, p45_stripes, p24_pieces, p4_grid, test_max_nb2;
} gk_test_part_in;
typedef struct gk_test_part_form { char name[16]; uint32_t chunk_keys, threads; uint64_t lds_bytes; } gk_test_part_form;
typedef struct gk_test_part_out {
    gk_test_part_form p4_op, p4_exact;
    char p2[16];
    int32_t supported, op1, fine_exact, sync_between, pipelined, stripes;
} gk_test_part_out;
int gk_test_part_plan(const gk_test_part_in *in, gk_test_part_out *out);

/* Which walker produced the last gk_graph_walk_pairs into `s`: *orientations = pair orientations handed to the walk stage (two per
 * pair whose mates both hold k bases), *overflowed = those of them whose sets outgrew the wave's LDS on the device and were walked
 * by the host walker instead (0 under "pairs_host" = 1, where the host walks all of them by choice).  Two host integers the call
 * leaves in the support; either pointer may be null.  A call that cut no pair leaves (0, 0). */
int gk_test_support_last_walk(const gk_support *s, uint64_t *orientations, uint64_t *overflowed);

/* The device scan every offset list of the library comes from (csrc/gk_scan.h: scan_counts, u32 counts in, u64 offsets out), run
 * on its own: in_host[0..n) is uploaded, out_host[0..n] receives the exclusive prefix sums and out_host[n] the total.
 * via_scratch = 0 takes the overload with the caller's scratch, sized to exactly the n / 4096 + 2 words callers give it;
 * via_scratch = 1 the overload that takes its scratch from the call's temporaries.  The result — and with via_scratch = 0 the
 * scratch — lies between guard regions of 64 words, before and after, and every word of the result starts as the guards'
 * pattern: *guard_hits = the guard words the scan changed (0 unless it wrote out of bounds; the second overload's own scratch
 * cannot be guarded).  n = 0 is legal (out_host[0] = 0, in_host may be null); any other null pointer is GK_E_INVALID. */
int gk_test_scan_counts(gk_ctx *ctx, const uint32_t *in_host, uint64_t n, int via_scratch, uint64_t *out_host, uint64_t *guard_hits);

/* The slot -> rank structure the pointer-jumping unitig build makes of a table (csrc/gk_graph.hip: k_rank_masks, k_rank_scan,
 * k_rank_fill, by the same function the build calls): for every block of 64 slots, masks[b] = its live slots and bases[b] = the
 * live slots before it; *total = the live slots the scan counted; *nblk = the blocks, ceil(slots / 64).  The graph phase only
 * ever reads the graph layout, so a count table of 8-byte keys is rebuilt into it first, exactly as gk_graph_build does (the
 * slot count stays unless the table is too dense for the graph phase); the map is otherwise unchanged and no graph is built.
 * GK_E_CAPACITY, with *nblk set and nothing copied, when cap_blocks < *nblk; GK_E_INVALID for a null pointer. */
int gk_test_slot_ranks(gk_map *map, uint64_t *masks, uint64_t *bases, uint64_t cap_blocks, uint64_t *nblk, uint64_t *total);

/* The canonical edge numbering by path content that gk_dist_reduce_links / gk_dist_reduce_spans use (include/genome_amd.h, "the
 * path key"; csrc/gk_links.hip: graph_edge_pathkeys, the same function), run on its own.  Every array has one entry per edge id
 * below gk_graph_id_bounds' edge bound: h1 / h2 = the key (2^64 - 1 twice for a dead edge), canon = the edge's place in the
 * canonical order (0xffffffff dead), dup = 1 where another live edge has the same key.  *nlive = the live edges, *fingerprint =
 * the replica's path fingerprint.  The hash kernel's grid honours "test_max_grid".  GK_E_INVALID for a null pointer. */
int gk_test_edge_path_keys(gk_graph *g, uint64_t *h1, uint64_t *h2, uint32_t *canon, uint8_t *dup, uint64_t *nlive, uint64_t *fingerprint);

/* gk_shard_superkmers_dev over a ragged stream: record r spans [dev_offsets[r], dev_offsets[r + 1]) of dev_records (nreads + 1
 * 32-bit offsets on the device; the records lie back to back, each 1 + ceil(len / 4) bytes with len its length byte, as a host
 * that walked the framing builds the table) and `windows` = the k-mer windows of all records.  It is the offset-table form of
 * the routing launch that only gk_dist_* reaches in the product (csrc/gk_skm.hip: skm_route_launch, the same function), followed
 * by the same wait and the same finish as gk_shard_superkmers_dev: regions, counts and GK_E_CAPACITY are as described there. */
int gk_test_skm_route_offsets(gk_ctx *ctx, int k, const void *dev_records, const uint32_t *dev_offsets, uint64_t nreads, uint64_t windows, int P,
                              void *dev_out, uint64_t out_cap_records, uint64_t *rec_counts_host, uint64_t *kmer_counts_host);

/* TEST transport: the ranks are threads of ONE process on ONE device; sends, receives and reductions go through a hub in the
 * library (device-to-device copies matched pairwise in posting order) instead of RCCL, which refuses two ranks on one GPU.  Every
 * rank passes the same 128 id bytes (any) and its own context; calls block until the peers have posted the matching operation
 * (an inconsistent order of operations across ranks deadlocks at once; a send and its receive that differ in size are GK_E_COMM).
 * Everything else about the handle is the product code path. */
int gk_dist_create_loopback(gk_ctx *ctx, int rank, int world, const void *id128, gk_dist **out);

#ifdef __cplusplus
}
#endif
#endif

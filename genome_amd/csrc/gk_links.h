// gk_links.h — what the N-rank reduces of the link and span tables (gk_dist_reduce_links / gk_dist_reduce_spans, gk_dist.hip)
// need of gk_links.hip and gk_spans.hip, as host calls that work on the context's stream: the canonical edge numbering BY PATH
// CONTENT of an edited graph, and a table's records as PLANES — a key plane (u64: the record's first two edge ids, e << 32 | f for
// a link, e << 32 | m for a span), a count plane (u32) and one extra plane (u64: a link's sum_u, a span's out-edge f) — which is
// the form in which records travel between ranks.  The kernels stay with their tables.
#pragma once

#include "gk_internal.h"

struct gk_graph;
struct gk_links;
struct gk_spans;

namespace gk {
// ---- the path key (the rule: include/genome_amd.h, "the path key"; tests/pathkey_ref.py restates it) ---------------------------
constexpr u64 PK_WORD = 0x70617468776f7264ULL, PK_SECOND = 0x7365636f6e64ULL, PK_H1 = 0x7061746831ULL, PK_H2 = 0x7061746832ULL;
constexpr u64 PK_GOLD = 0x9e3779b97f4a7c15ULL, PK_FP = 0x66696e676572ULL, PK_LIVE = 0x6c697665ULL;
constexpr u32 PK_CHUNK_WORDS = 64;                     // words of 32 bases one wave step takes: the unit of one atomic add per (edge, chunk)
GK_HD u64 pk_fold(u64 acc, u64 v) { return mix64(acc ^ (v + PK_GOLD)); }
// the two terms word j of an edge's sequence adds to the edge's sums
GK_HD void pk_word_terms(u64 word, u64 j, u64 *t1, u64 *t2) {
    const u64 t = word ^ mix64(j + PK_WORD);
    *t1 = mix64(t);
    *t2 = mix64(t ^ PK_SECOND);
}
GK_HD void pk_finish(u64 s1, u64 s2, u64 lo, u64 hi, u64 len, u64 *h1, u64 *h2) {
    const u64 a = pk_fold(pk_fold(pk_fold(pk_fold(PK_H1, s1), lo), hi), len);
    *h1 = a == ~0ull ? a - 1 : a;                       // (~0 sorts the dead edges last)
    *h2 = pk_fold(pk_fold(pk_fold(pk_fold(PK_H2, s2), lo), hi), len);
}

// The canonical edge numbering of an EDITED replica: live edges ordered by their path key (h1, h2) — a function of the path
// P(e) = start k-mer ++ seq alone, so the same on every replica that holds the same paths, whatever ids and pool places its
// edits gave them.  *d_canon [n_edges]: local id -> canonical (0xffffffff dead), *d_inv [*nlive]: canonical -> local id,
// *d_dup [n_edges]: 1 where another live edge has the same key (the two are neighbours in the order); all three belong to
// `keep`.  *content_fp: equal on two replicas iff they hold the same multiset of paths.  d_h1 / d_h2 (optional, [n_edges], in
// `keep`): the keys themselves (~0, ~0 for a dead edge).  One streaming pass over the live words of the pool (no copy of it),
// one atomic add per (edge, 64-word chunk); the sorts are rocPRIM's radix sort.
int graph_edge_pathkeys(gk_graph *g, DevScratch &keep, u32 **d_canon, u32 **d_inv, uint8_t **d_dup, u64 *nlive, u64 *content_fp, u64 **d_h1 = nullptr,
                        u64 **d_h2 = nullptr);

// ---- records as planes ---------------------------------------------------------------------------------------------------------
struct RecPlanes { u64 *key = nullptr; u32 *cnt = nullptr; u64 *x = nullptr; };
// What the exchange needs of a table type T (gk_links, gk_spans): rec_distinct (its distinct records); rec_bucket (its records
// grouped by owner rank, as support_bucket does: region[0..P], `room` records must fit; canon / dup / nmap: the records leave in
// the canonical numbering, GK_E_STATE if one names an edge that is dead or a duplicate there; the owner is a hash of the key
// plane, so a span's (e, m) has one owner whatever f); rec_insert (n records into t, checked: *overflow if a count passes
// 2^32-1); rec_uncanon (planes back to this replica's ids, in place); rec_new / rec_free (an empty table with room for `want`);
// rec_adopt (s takes t's contents, t gets s's: called once nothing can fail any more).
template <class T> int rec_distinct(const T *t, u64 *n);
template <class T> int rec_bucket(T *t, int P, const RecPlanes &out, u64 room, u64 *region, const u32 *canon, const uint8_t *dup, u64 nmap);
template <class T> int rec_insert(T *t, const RecPlanes &in, u64 n, bool *overflow);
template <class T> int rec_uncanon(gk_ctx *ctx, const RecPlanes &p, u64 n, const u32 *d_inv, u64 nlive);
template <class T> int rec_new(gk_ctx *ctx, u64 want, u64 id_bound, T **out);
template <class T> void rec_free(T *t);
template <class T> int rec_adopt(T *s, T *t);
template <class T> gk_ctx *rec_ctx(const T *t);
}  // namespace gk

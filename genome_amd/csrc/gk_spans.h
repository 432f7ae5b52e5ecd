// gk_spans.h — the span table (gk_spans: (in-edge e, spanned edge m, out-edge f) -> reads that cross m from end to end) as the
// translation units that are not gk_spans.hip see it: the edge split (gk_graph_split_edges_by_spans, gk_pairs.hip) reads it on
// the host.
#pragma once

#include <vector>

#include "gk_internal.h"

// A key is (e << 33 | m << 2 | slot): edge ids are below 2^31 - 1, so no key is SUP_EMPTY (~0).  The out-edge f does not fit the
// key; it lies in a plane of its own, and `slot` numbers the at most four f behind one (e, m) in the order they arrived.
// ctr: [0] distinct triples [3] table full [4] a count passed 2^32-1 [5] a fifth out-edge behind one (e, m)
struct SpanView { gk::u64 *keys; gk::u32 *f; gk::u32 *cnt; gk::u64 mask; unsigned long long *ctr; };
struct gk_spans {
    gk_ctx *ctx = nullptr;
    gk::u64 *d_keys = nullptr;                 // open addressing, power-of-two capacity
    gk::u32 *d_f = nullptr;                    // 0xffffffff until the slot's first triple has written it
    gk::u32 *d_cnt = nullptr;
    gk::u64 cap = 0;
    unsigned long long *d_ctr = nullptr;       // 8 words (SpanView::ctr)
};

namespace gk {
// the triples of s on the host, in slot order
int spans_to_host(const gk_spans *s, std::vector<u32> &e, std::vector<u32> &m, std::vector<u32> &f, std::vector<u32> &count);
}

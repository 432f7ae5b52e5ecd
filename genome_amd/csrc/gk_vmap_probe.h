// gk_vmap_probe.h — the value map's probe (Container.getAll, S/ds/ArrayDNAMap.scala:103-113) as device code that more than one
// translation unit runs: gk_vmap.hip (k_vm_get_all) and gk_thread.hip (k_thread_reads).  It is the one place that knows how a
// multimap key is found in the three slot layouts of gk_device.h, k = 64's tag-in-address stride included.
#pragma once

#include "gk_device.h"

namespace gk {

template <int W> __device__ __forceinline__ void slot_set_value(Slot<W> *s, u64 v) { s->extra = (u32)v; s->aux = (u32)(v >> 32); }
template <int W> __device__ __forceinline__ u64 slot_value(const Slot<W> *s) { return (u64)s->extra | ((u64)s->aux << 32); }

// a 128-bit key is visible only once BOTH words are in place (seg_claim_unique writes w0 then w1): a reader that meets a slot
// whose w0 matches and whose w1 is still EMPTY is looking at an insert of ANOTHER launch phase, which these maps never overlap
// with lookups (handles are externally synchronised), so plain loads suffice here.
template <int W> __device__ __forceinline__ bool slot_has_key(const Slot<W> *s, Kmer<W> key, u32 tagged, u64 index) {
    if constexpr (W == 1) return s->w0 == key.lo;
    else {
        const Stored<2> k = to_stored(key);
        return s->w0 == k.w0 && s->w1 == k.w1 && (!tagged || (u32)(index & 3u) == key_tag(key));
    }
}

// Walk the key's probe sequence to the first free slot; f(value, j) for the j-th slot that holds the key, in probe order, until
// `limit` of them were seen.  Returns how many were.
template <int W, class F> __device__ __forceinline__ u32 vmap_for_each(const Table<W> &t, Kmer<W> key, u32 limit, F f) {
    constexpr u32 smask = (1u << SegBits<W>::value) - 1u;
    const u64 h = slot_hash(key);
    const u64 base = (u64)seg_of(t, h) << SegBits<W>::value;
    const Slot<W> *seg = t.slots + base;
    const u32 step = t.tagged ? 4u : 1u;
    u32 p = t.tagged ? ((seg_pos<W>(h) & ~3u) | key_tag(key)) : seg_pos<W>(h);
    u32 found = 0;
    for (u32 s = 0; s <= smask && found < limit; s += step) {
        if (seg[p].w0 == KEY_EMPTY) break;
        if (slot_has_key(&seg[p], key, t.tagged, base + p)) {
            f(slot_value(&seg[p]), found);
            found++;
        }
        p = (p + step) & smask;
    }
    return found;
}

// How many entries the key has — 0, 1, or 2 for "two or more" — and, if one, its value in *value (with more, the first in probe order).
template <int W> __device__ __forceinline__ u32 vmap_count_one(const Table<W> &t, Kmer<W> key, u64 *value) {
    return vmap_for_each(t, key, 2u, [&](u64 v, u32 j) { if (j == 0) *value = v; });
}

}  // namespace gk

// gk_fasta.hip — every k-window of a FASTA text looked up in a position map on the device: the loop of CheckGraph
// (S/scripts/CheckGraph.scala:48-55).  The rules, with this check's deviations, are in include/genome_amd.h ("FASTA check").
//
// One device slice = the next piece of the caller's text (no text is carried between slices; the carry is the last k-1 squeezed
// codes with their positions and covered flags, "inside a header", the line and column counters):
//   k_fq_terms (pass 0, 1)   gk_text.h: terminators per 16 KiB tile, then their positions E[line] = end of line
//   k_fa_squeeze (pass 0)    the same tiles, a wave per 4 KiB: kept characters per wave (headers and terminators are dropped)
//   scan_counts              kept counts -> where each wave writes
//   k_fa_squeeze (pass 1)    one code per kept character: 0..3 a base, 4 an invalid character, 5 a break ('>' of a header; a
//                            terminator in per_line mode); optionally the text position of each code; the text counters
//   k_fa_short               one lane per terminator: non-header lines of 1..k-1 characters
//   k_fa_windows             the stream [carried codes | squeezed codes] staged in LDS with a k-1 halo; a lane owns 16 consecutive
//                            start positions, rolls the k-mer with append_base, probes the table for each window of k valid codes
//                            (gk_vmap.hip's `contains`: ~1.3 random 64-byte sectors per lookup, the HBM random-access rate is the
//                            bound); one bit per start in a window bitmap and a found bitmap; counters by one atomic per wave
//   k_fa_cover               found bitmap dilated by k = covered positions; the positions that are not carried on are counted
//   k_fa_miss_count / scan_counts / k_fa_miss_emit     ordered compaction of (window & ~found): the first max_missing entries
//   k_fa_carry               the last k-1 codes, their covered flags and positions; the line / column state of the next slice
// Windows that start inside the last k-1 codes of a slice are evaluated by the next slice (or never, at the end of the input:
// they have no k-th code), so every start position is evaluated once and every position is counted as covered once.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>

#include "gk_text.h"

struct gk_vmap;
namespace gk {
int vmap_k(const gk_vmap *m);
gk_ctx *vmap_ctx(const gk_vmap *m);
void vmap_table(const gk_vmap *m, void **slots, uint32_t *nb2, uint32_t *lnb1);
}

namespace {

constexpr u64 FA_SLICE_DEFAULT = 64ull << 20;           // text bytes per device slice (E and the position array index a slice by u32)
constexpr u32 FA_HEAD = 64;                             // room in front of the squeezed codes for the carried ones (<= 63)
constexpr u32 FA_RUN = 16;                              // consecutive start positions per lane of k_fa_windows
constexpr u32 FA_WT = 256 * FA_RUN;                     // start positions per workgroup
constexpr u32 FA_WAVES = FQ_BLOCK / 64;
constexpr u64 FA_NONE = ~0ull;
enum : u32 { FA_INVALID = 4, FA_BREAK = 5 };

struct FaState {                 // device resident; the first 14 words are what the host reads after every feed
    unsigned long long line;                 // terminators so far = 0-based line of the next byte
    unsigned long long tail_line;            // 1: the input ended in an unterminated non-empty line (k_fa_finish)
    unsigned long long headers, bases, valid_bases, windows, found, covered, short_lines;
    unsigned long long first_hdr, first_seq; // offset in the whole input of the first header / the first sequence character
    unsigned long long nmiss;                // entries of the missing list
    unsigned long long col;                  // characters of the line in progress
    unsigned long long carry_cov;            // bit i: carried code i already lies inside a found window
    u32 in_header;                           // col > 0: the line in progress is a header
    u32 nc;                                  // carried codes
    uint8_t code[64];
    unsigned long long c_off[64], c_line[64], c_col[64];    // where each carried code stands in the input
};
constexpr size_t FA_STATE_HOST = 14 * 8;

struct FaSlice {                 // one slice's arrays, by value to the kernels
    const uint8_t *T;            // text
    u64 n;                       // its bytes
    u64 text_off;                // offset of T[0] in the whole input
    const u32 *E;                // terminator positions
    u64 terms;
    const uint8_t *S;            // the stream: carried codes, then this slice's squeezed codes
    u64 Ltot, P;                 // its length; start positions evaluated now (Ltot - k + 1, or 0)
    const u32 *src;              // text position of each squeezed code (nullptr: no missing list wanted)
};

__device__ __forceinline__ u64 fa_wave_sum(u64 v) {
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d);
    return v;
}

// pass 0: kept characters per wave (4 KiB of text); pass 1: their codes at kept_off[wave], and the text counters
template <int PASS>
__global__ __launch_bounds__(FQ_BLOCK) void k_fa_squeeze(const uint8_t *__restrict__ T, u64 n, u64 text_off, const u32 *__restrict__ E,
                                                          const unsigned long long *__restrict__ term_off, int per_line, FaState *st,
                                                          u32 *__restrict__ wave_kept, const unsigned long long *__restrict__ kept_off,
                                                          uint8_t *__restrict__ codes, u32 *__restrict__ src) {
    __shared__ u32 s_tile[(FQ_TILE + 64) / 4];
    __shared__ u32 s_has[FA_WAVES], s_hdr[FA_WAVES];
    const u64 g0 = (u64)blockIdx.x * FQ_TILE, g1 = umin(n, g0 + FQ_TILE);
    const u64 a0 = stage_tile(s_tile, T, g0 ? g0 - 1 : 0, g1);
    __syncthreads();
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(s_tile);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr u32 PER_WAVE = FQ_TILE / FA_WAVES;
    const u64 w0 = g0 + (u64)wave * PER_WAVE;
    const u64 col0 = st->col;
    // is the line that runs into this tile a header?  (the terminator count before the tile is the line index of its first byte)
    const u64 jl = term_off[blockIdx.x];
    bool tile_hdr = false;
    if (jl == 0) tile_hdr = col0 > 0 ? st->in_header != 0 : (g0 > 0 && T[0] == '>');
    else {
        const u64 start = fq_line_start(T, n, E, jl);
        if (start < g0) tile_hdr = T[start] == '>';
    }
    // a line starts at x: after "\n", after a '\r' that no '\n' follows, or at the slice's first byte when no line is in progress
    auto line_start = [&](u64 x, u32 c) -> bool {
        if (x == 0) return col0 == 0;
        const u32 p = tb[x - 1 - a0];
        return p == '\n' || (p == '\r' && c != '\n');
    };
    // the header state each wave starts in: the last line start before it decides
    u32 has = 0, h = 0;
    for (u32 s = 0; s < PER_WAVE; s += 64) {
        const u64 x = w0 + s + lane;
        const u32 c = x < g1 ? tb[x - a0] : 0u;
        const bool ls = x < g1 && line_start(x, c);
        const unsigned long long m_ls = __ballot(ls), m_hs = __ballot(ls && c == '>');
        if (m_ls) { has = 1; h = (u32)((m_hs >> (63 - __clzll((long long)m_ls))) & 1ull); }
    }
    if (lane == 0) { s_has[wave] = has; s_hdr[wave] = h; }
    __syncthreads();
    u32 hdr = tile_hdr ? 1u : 0u;
    for (int w = 0; w < wave; w++) if (s_has[w]) hdr = s_hdr[w];
    const unsigned long long below = (1ull << lane) - 1ull, upto = below | (1ull << lane);
    u64 o = PASS ? kept_off[(u64)blockIdx.x * FA_WAVES + wave] : 0;
    u32 cnt = 0, nb = 0, nv = 0, nh = 0;
    u64 fh = FA_NONE, fs = FA_NONE;
    for (u32 s = 0; s < PER_WAVE; s += 64) {
        const u64 x = w0 + s + lane;
        const bool in = x < g1;
        const u32 c = in ? tb[x - a0] : 0u;
        const bool lf2 = in && c == '\n' && x > 0 && tb[x - 1 - a0] == '\r';
        const bool term = in && (c == '\r' || (c == '\n' && !lf2));
        const bool ls = in && line_start(x, c);
        const unsigned long long m_ls = __ballot(ls), m_hs = __ballot(ls && c == '>');
        const unsigned long long mine = m_ls & upto;
        const bool my_hdr = mine ? ((m_hs >> (63 - __clzll((long long)mine))) & 1ull) != 0 : hdr != 0;
        int code = -1;
        if (in && !lf2) {
            if (term) code = per_line ? (int)FA_BREAK : -1;
            else if (my_hdr) code = (ls && c == '>') ? (int)FA_BREAK : -1;
            else code = c == 'A' ? 0 : c == 'G' ? 1 : c == 'C' ? 2 : c == 'T' ? 3 : (int)FA_INVALID;
        }
        const unsigned long long m_keep = __ballot(code >= 0);
        if (PASS == 0) cnt += (u32)__popcll(m_keep);
        else {
            if (code >= 0) {
                const u64 at = o + (u64)__popcll(m_keep & below);
                codes[at] = (uint8_t)code;
                if (src) src[at] = (u32)x;
            }
            o += (u64)__popcll(m_keep);
            const unsigned long long m_seq = __ballot(code >= 0 && code <= (int)FA_INVALID);
            nb += (u32)__popcll(m_seq);
            nv += (u32)__popcll(__ballot(code >= 0 && code < (int)FA_INVALID));
            nh += (u32)__popcll(m_hs);
            if (m_hs && fh == FA_NONE) fh = text_off + w0 + s + (u64)(__ffsll((long long)m_hs) - 1);
            if (m_seq && fs == FA_NONE) fs = text_off + w0 + s + (u64)(__ffsll((long long)m_seq) - 1);
        }
        if (m_ls) hdr = (u32)((m_hs >> (63 - __clzll((long long)m_ls))) & 1ull);
    }
    if (lane != 0) return;
    if (PASS == 0) { wave_kept[(u64)blockIdx.x * FA_WAVES + wave] = cnt; return; }
    if (nb) atomicAdd(&st->bases, (unsigned long long)nb);
    if (nv) atomicAdd(&st->valid_bases, (unsigned long long)nv);
    if (nh) atomicAdd(&st->headers, (unsigned long long)nh);
    if (fh != FA_NONE) atomicMin(&st->first_hdr, (unsigned long long)fh);
    if (fs != FA_NONE) atomicMin(&st->first_seq, (unsigned long long)fs);
}

// one lane per terminator: the line it ends is short if it is no header and has 1..k-1 characters
__global__ __launch_bounds__(FQ_BLOCK) void k_fa_short(const uint8_t *__restrict__ T, u64 n, const u32 *__restrict__ E, u64 terms, int k, FaState *st) {
    const u64 j = (u64)blockIdx.x * FQ_BLOCK + threadIdx.x;
    u64 is_short = 0;
    if (j < terms) {
        const u64 e = E[j], start = fq_line_start(T, n, E, j), col0 = j == 0 ? st->col : 0;
        const u64 len = e - start + col0;
        const bool hdr = col0 > 0 ? st->in_header != 0 : (len > 0 && T[start] == '>');
        is_short = (!hdr && len >= 1 && len < (u64)k) ? 1 : 0;
    }
    is_short = fa_wave_sum(is_short);
    if ((threadIdx.x & 63) == 0 && is_short) atomicAdd(&st->short_lines, (unsigned long long)is_short);
}

__global__ void k_fa_put_carry(const FaState *st, uint8_t *codes, u32 nc) {
    if (threadIdx.x < nc) codes[FA_HEAD - nc + threadIdx.x] = st->code[threadIdx.x];
}

// `contains` (CheckGraph.scala:51) for every window of k valid codes; bit r of a lane's word = start position p + r
template <int W>
__global__ __launch_bounds__(256) void k_fa_windows(Table<W> t, int k, const uint8_t *__restrict__ S, u64 Ltot, u64 P, uint16_t *__restrict__ wbits,
                                                    uint16_t *__restrict__ fbits, u64 nshort, FaState *st) {
    __shared__ u32 s_code[(FA_WT + 128) / 4];
    const u64 pb = (u64)blockIdx.x * FA_WT;
    const u64 cend = umin(Ltot, pb + FA_WT + (u64)k - 1);
    u64 a0 = 0;
    if (pb < cend) a0 = stage_tile(s_code, S, pb, cend);
    __syncthreads();
    const uint8_t *sc = reinterpret_cast<const uint8_t *>(s_code);
    const u64 p = pb + (u64)threadIdx.x * FA_RUN;
    u32 wm = 0, fm = 0;
    if (p < P) {
        Kmer<W> km{};
        u32 good = 0;
        for (int j = 0; j < k - 1; j++) {
            const u32 c = sc[p + j - a0];
            km = append_base(km, (int)(c & 3u), k);
            good = c < FA_INVALID ? good + 1 : 0;
        }
        for (u32 r = 0; r < FA_RUN && p + r < P; r++) {
            const u32 c = sc[p + r + k - 1 - a0];
            km = append_base(km, (int)(c & 3u), k);
            good = c < FA_INVALID ? good + 1 : 0;
            if (good >= (u32)k) {
                wm |= 1u << r;
                if (table_find(t, km) >= 0) fm |= 1u << r;
            }
        }
    }
    const u64 idx = (u64)blockIdx.x * 256 + threadIdx.x;
    if (idx < nshort) { wbits[idx] = (uint16_t)wm; fbits[idx] = (uint16_t)fm; }
    const u64 nw = fa_wave_sum((u64)__popc(wm)), nf = fa_wave_sum((u64)__popc(fm));
    if ((threadIdx.x & 63) == 0) {
        if (nw) atomicAdd(&st->windows, (unsigned long long)nw);
        if (nf) atomicAdd(&st->found, (unsigned long long)nf);
    }
}

// C = F dilated by k: position i is covered if a found window starts in [i - k + 1, i]; the carried codes bring their flags.
// Positions below P are final (every start that can cover them has been evaluated): they are counted; the rest is carried.
__global__ __launch_bounds__(256) void k_fa_cover(const unsigned long long *__restrict__ F, u64 nF, u64 nC, u64 P, int k, unsigned long long *__restrict__ C,
                                                  FaState *st) {
    u64 cnt = 0;
    for (u64 w = (u64)blockIdx.x * 256 + threadIdx.x; w < nC; w += (u64)gridDim.x * 256) {
        unsigned long long lo = (w >= 1 && w - 1 < nF) ? F[w - 1] : 0ull, hi = w < nF ? F[w] : 0ull;
        for (int len = 1; len < k;) {
            const int s = min(len, k - len);                 // 1..32
            const unsigned long long nhi = hi | (hi << s) | (lo >> (64 - s));
            lo |= lo << s;
            hi = nhi;
            len += s;
        }
        if (w == 0) hi |= st->carry_cov;
        C[w] = hi;
        const u64 b0 = w * 64;
        const unsigned long long mask = b0 + 64 <= P ? ~0ull : b0 >= P ? 0ull : ((1ull << (P - b0)) - 1ull);
        cnt += (u64)__popcll(hi & mask);
    }
    cnt = fa_wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&st->covered, (unsigned long long)cnt);
}

__global__ __launch_bounds__(256) void k_fa_miss_count(const unsigned long long *__restrict__ Wb, const unsigned long long *__restrict__ F, u64 nF,
                                                       u32 *__restrict__ cnt) {
    for (u64 w = (u64)blockIdx.x * 256 + threadIdx.x; w < nF; w += (u64)gridDim.x * 256) cnt[w] = (u32)__popcll(Wb[w] & ~F[w]);
}

// where stream position p stands in the input: offset, 0-based line and column
__device__ __forceinline__ void fa_pos(const FaSlice &sl, const FaState *st, u32 nc, u64 p, u64 *off, u64 *line, u64 *col) {
    if (p < nc) { *off = st->c_off[p]; *line = st->c_line[p]; *col = st->c_col[p]; return; }
    const u64 pos = sl.src[p - nc];
    u64 lo = 0, hi = sl.terms;                           // terminators in front of pos
    while (lo < hi) { const u64 mid = (lo + hi) / 2; if (sl.E[mid] < pos) lo = mid + 1; else hi = mid; }
    *off = sl.text_off + pos;
    *line = st->line + lo;
    *col = lo ? pos - fq_line_start(sl.T, sl.n, sl.E, lo) : st->col + pos;
}

// ordered compaction: word w's not-found windows take list entries have + moff[w] ..., in bit order
__global__ __launch_bounds__(256) void k_fa_miss_emit(FaSlice sl, const FaState *st, u32 nc, int k, const unsigned long long *__restrict__ Wb,
                                                      const unsigned long long *__restrict__ F, u64 nF, const unsigned long long *__restrict__ moff,
                                                      u64 have, u64 max_missing, unsigned long long *__restrict__ m_off, unsigned long long *__restrict__ m_line,
                                                      unsigned long long *__restrict__ m_col, unsigned long long *__restrict__ m_lo, unsigned long long *__restrict__ m_hi) {
    for (u64 w = (u64)blockIdx.x * 256 + threadIdx.x; w < nF; w += (u64)gridDim.x * 256) {
        u64 at = have + moff[w];
        unsigned long long m = Wb[w] & ~F[w];
        while (m && at < max_missing) {
            const u64 p = w * 64 + (u64)(__ffsll((long long)m) - 1);
            m &= m - 1;
            u64 lo = 0, hi = 0;
            for (int j = 0; j < k; j++) {
                const u64 c = sl.S[p + j] & 3u;
                if (j < 32) lo |= c << (2 * j); else hi |= c << (2 * (j - 32));
            }
            u64 off, line, col;
            fa_pos(sl, st, nc, p, &off, &line, &col);
            m_off[at] = off; m_line[at] = line; m_col[at] = col; m_lo[at] = lo; m_hi[at] = hi;
            at++;
        }
    }
}

// one wave: the last min(k - 1, Ltot) codes are carried on with their covered flags and positions; then the line state moves
// past the slice
__global__ __launch_bounds__(64) void k_fa_carry(FaSlice sl, FaState *st, u32 nc, u32 nc_new, const unsigned long long *__restrict__ C, u64 appended) {
    const u32 lane = threadIdx.x;
    u32 code = 0;
    u64 off = 0, line = 0, col = 0;
    bool cov = false;
    if (lane < nc_new) {
        const u64 p = sl.Ltot - nc_new + lane;
        code = sl.S[p];
        cov = ((C[p >> 6] >> (p & 63)) & 1ull) != 0;
        if (sl.src) fa_pos(sl, st, nc, p, &off, &line, &col);
    }
    const unsigned long long m_cov = __ballot(cov);
    __syncthreads();
    if (lane < nc_new) { st->code[lane] = (uint8_t)code; st->c_off[lane] = off; st->c_line[lane] = line; st->c_col[lane] = col; }
    if (lane != 0) return;
    st->carry_cov = m_cov;
    st->nc = nc_new;
    st->nmiss += appended;
    if (sl.terms == 0) {
        if (sl.n && st->col == 0) st->in_header = sl.T[0] == '>' ? 1u : 0u;
        st->col += sl.n;
    } else {
        const u64 start = fq_line_start(sl.T, sl.n, sl.E, sl.terms);
        st->col = sl.n - start;
        st->in_header = (start < sl.n && sl.T[start] == '>') ? 1u : 0u;
        st->line += sl.terms;
    }
}

// end of the input: an unterminated non-empty tail is a line; the carried codes start no window, their covered flags are final
__global__ void k_fa_finish(FaState *st, int k) {
    if (st->col > 0) {
        st->tail_line = 1;
        if (!st->in_header && st->col < (unsigned long long)k) st->short_lines += 1;
    }
    st->covered += (unsigned long long)__popcll(st->carry_cov);
    st->carry_cov = 0;
    st->nc = 0;
}

}  // namespace

struct gk_fasta_check {
    gk_ctx *ctx = nullptr;
    gk_vmap *vm = nullptr;
    int k = 0, W = 1, per_line = 0;
    u64 max_missing = 0;
    bool failed = false, finished = false;
    bool prev_cr = false;                     // the last byte consumed was '\r': a '\n' that follows belongs to the same terminator
    u64 text_off = 0;                         // bytes consumed
    u32 nc = 0;                               // carried codes (mirror of FaState::nc)
    u64 have = 0;                             // entries of the missing list (mirror of FaState::nmiss)
    FaState *d_st = nullptr;
    unsigned long long *d_miss = nullptr;     // five arrays of miss_cap entries: offset, line, column, lo, hi
    u64 miss_cap = 0;
    unsigned long long *h = nullptr;          // pinned: [0..13] FaState's counters, [14] terminators, [15] kept characters
    TextUpload up;                            // the copy-stream upload of a slice (gk_text.h)
    float ms[4] = {0, 0, 0, 0};
};

namespace {

int fa_fail(gk_fasta_check *fc, int code, const std::string &msg) {
    fc->failed = true;
    return fail(fc->ctx, code, msg);
}
#define FA_HIP(fc, call)                                                                        \
    do {                                                                                        \
        hipError_t e__ = (call);                                                                \
        if (e__ != hipSuccess) { (fc)->failed = true; return gk::hip_fail((fc)->ctx, e__, #call); } \
    } while (0)

u64 fa_slice_max(const gk_fasta_check *fc) { return fc->ctx->hook_fastq_chunk > 0 ? (u64)fc->ctx->hook_fastq_chunk : FA_SLICE_DEFAULT; }

// the missing list holds at least `want` entries (the five arrays move together)
int fa_miss_reserve(gk_fasta_check *fc, u64 want) {
    if (fc->miss_cap >= want) return GK_OK;
    gk_ctx *ctx = fc->ctx;
    const u64 cap = std::min<u64>(fc->max_missing, std::max<u64>(want, fc->miss_cap * 2));
    unsigned long long *nm = nullptr;
    FA_HIP(fc, pool_malloc(ctx, &nm, cap * 5 * 8));
    for (int a = 0; a < 5 && fc->have; a++)
        FA_HIP(fc, hipMemcpyAsync(nm + a * cap, fc->d_miss + a * fc->miss_cap, fc->have * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (fc->d_miss) FA_HIP(fc, pool_free(ctx, fc->d_miss));        // (waits for the context's streams: the moves have landed)
    fc->d_miss = nm;
    fc->miss_cap = cap;
    return GK_OK;
}

struct FaCut { u64 begin, len; };
// the next slice of text [pos, nbytes): a '\n' right after a '\r' is the second half of that terminator and is stepped over
FaCut fa_cut(const char *text, u64 nbytes, u64 pos, bool prev_cr, u64 slice_max) {
    if (pos < nbytes && text[pos] == '\n' && (pos ? text[pos - 1] == '\r' : prev_cr)) pos++;
    return FaCut{pos, std::min<u64>(nbytes - pos, slice_max)};
}

template <class T> T *fa_carve(uint8_t *&at, u64 n) {
    T *p = reinterpret_cast<T *>(at);
    at += (n * sizeof(T) + 255) & ~255ull;
    return p;
}

int fa_run(gk_fasta_check *fc, const char *text, u64 nbytes) {
    gk_ctx *ctx = fc->ctx;
    const int k = fc->k;
    double up_ms = 0, parse_ms = 0, look_ms = 0;
    const bool pinned = TextUpload::is_pinned(text);
    const u64 slice_max = fa_slice_max(fc);
    const bool want_pos = fc->max_missing > 0;
    // every buffer of the call in one pooled block, carved (sizes for the largest slice)
    const u64 cap = std::min<u64>(nbytes, slice_max), ntiles_max = (cap + FQ_TILE - 1) / FQ_TILE, nwv = ntiles_max * FA_WAVES;
    const u64 nbits = (cap + FA_HEAD) / 64 + 2;                      // words of a bitmap over the stream
    const u64 nscan = std::max<u64>(nwv, nbits) / SCAN_CHUNK + 4;
    const int nbuf = nbytes > cap ? 2 : 1;
    const bool e_in_block = cap <= (4ull << 20);                     // small slices: the line ends live in the block too (at most one per byte)
    auto layout = [&](uint8_t *base, uint8_t **tb, uint8_t **codes, u32 **src, u32 **tile_cnt, unsigned long long **tile_off, u32 **wave_kept,
                      unsigned long long **kept_off, u64 **scan, unsigned long long **wb, unsigned long long **fb, unsigned long long **cb, u32 **mcnt,
                      unsigned long long **moff, u32 **eblk) -> u64 {
        uint8_t *at = base;
        for (int i = 0; i < nbuf; i++) tb[i] = fa_carve<uint8_t>(at, cap + 64);
        *codes = fa_carve<uint8_t>(at, cap + FA_HEAD + 128);
        *src = want_pos ? fa_carve<u32>(at, cap + 1) : nullptr;
        *tile_cnt = fa_carve<u32>(at, ntiles_max + 1);
        *tile_off = fa_carve<unsigned long long>(at, ntiles_max + 2);
        *wave_kept = fa_carve<u32>(at, nwv + 1);
        *kept_off = fa_carve<unsigned long long>(at, nwv + 2);
        *scan = fa_carve<u64>(at, nscan);
        *wb = fa_carve<unsigned long long>(at, nbits);
        *fb = fa_carve<unsigned long long>(at, nbits);
        *cb = fa_carve<unsigned long long>(at, nbits);
        *mcnt = want_pos ? fa_carve<u32>(at, nbits + 1) : nullptr;
        *moff = want_pos ? fa_carve<unsigned long long>(at, nbits + 2) : nullptr;
        *eblk = e_in_block ? fa_carve<u32>(at, cap + 2) : nullptr;
        return std::max<u64>((u64)(at - base), 1ull << 20);         // (a block of 1 MiB is pooled: a stream of tiny feeds reuses it)
    };
    uint8_t *tb[2] = {nullptr, nullptr}, *codes = nullptr;
    u32 *src = nullptr, *tile_cnt = nullptr, *wave_kept = nullptr, *mcnt = nullptr, *eblk = nullptr;
    unsigned long long *tile_off = nullptr, *kept_off = nullptr, *wb = nullptr, *fb = nullptr, *cb = nullptr, *moff = nullptr;
    u64 *scan = nullptr;
    const u64 total = layout(nullptr, tb, &codes, &src, &tile_cnt, &tile_off, &wave_kept, &kept_off, &scan, &wb, &fb, &cb, &mcnt, &moff, &eblk);
    DevScratch tmp(ctx);
    uint8_t *block = nullptr;
    FA_HIP(fc, tmp.get(&block, total));
    layout(block, tb, &codes, &src, &tile_cnt, &tile_off, &wave_kept, &kept_off, &scan, &wb, &fb, &cb, &mcnt, &moff, &eblk);

    void *slots = nullptr;
    uint32_t nb2 = 1, lnb1 = 0;
    vmap_table(fc->vm, &slots, &nb2, &lnb1);
    const TimedSection kt{ctx};
    int rc = GK_OK;
    int b = 0;
    FaCut cut = fa_cut(text, nbytes, 0, fc->prev_cr, slice_max);
    bool uploaded = false;                                           // the current slice is already on its way into tb[b]
    while (cut.len) {
        const u64 n = cut.len;
        if (!uploaded) { if ((rc = fc->up.upload(ctx, b, tb[b], text + cut.begin, n, pinned, &up_ms))) { fc->failed = true; return rc; } }
        FA_HIP(fc, hipStreamWaitEvent(ctx->stream, fc->up.up1[b], 0));
        const uint8_t *T = tb[b];
        const u64 slice_off = fc->text_off + cut.begin;              // offset of T[0] in the whole input (text_off: before this call)
        const u64 ntiles = (n + FQ_TILE - 1) / FQ_TILE;
        // ---- line ends
        FA_HIP(fc, kt.start());
        hipLaunchKernelGGL((k_fq_terms<0>), dim3((unsigned)ntiles), dim3(FQ_BLOCK), 0, ctx->stream, T, n, tile_cnt, nullptr, nullptr);
        FA_HIP(fc, hipGetLastError());
        FA_HIP(fc, scan_counts(ctx, tile_cnt, ntiles, tile_off, scan));
        FA_HIP(fc, hipMemcpyAsync(&fc->h[14], tile_off + ntiles, 8, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = kt.end(&parse_ms))) { fc->failed = true; return rc; }
        const u64 terms = fc->h[14];
        {
            float t = 0;
            FA_HIP(fc, hipEventElapsedTime(&t, fc->up.up0[b], fc->up.up1[b]));
            up_ms += t;
        }
        if (terms > n) return fa_fail(fc, GK_E_STATE, "gk_fasta_check: more line ends than characters (internal error)");
        u32 *E = eblk;
        if (!E) FA_HIP(fc, tmp.get(&E, terms + 2));
        // ---- squeeze
        FA_HIP(fc, kt.start());
        hipLaunchKernelGGL((k_fq_terms<1>), dim3((unsigned)ntiles), dim3(FQ_BLOCK), 0, ctx->stream, T, n, nullptr, tile_off, E);
        hipLaunchKernelGGL((k_fa_squeeze<0>), dim3((unsigned)ntiles), dim3(FQ_BLOCK), 0, ctx->stream, T, n, slice_off, E, tile_off, fc->per_line, fc->d_st,
                           wave_kept, nullptr, nullptr, nullptr);
        FA_HIP(fc, hipGetLastError());
        FA_HIP(fc, scan_counts(ctx, wave_kept, ntiles * FA_WAVES, kept_off, scan));
        FA_HIP(fc, hipMemcpyAsync(&fc->h[15], kept_off + ntiles * FA_WAVES, 8, hipMemcpyDeviceToHost, ctx->stream));
        // (the next slice goes up on the copy stream beside the rest of this one: the other text buffer is free)
        const FaCut next = fa_cut(text, nbytes, cut.begin + n, false, slice_max);
        if (next.len) { if ((rc = fc->up.upload(ctx, 1 - b, tb[1 - b], text + next.begin, next.len, pinned, &up_ms))) { fc->failed = true; return rc; } }
        if ((rc = kt.end(&parse_ms))) { fc->failed = true; return rc; }
        const u64 m = fc->h[15];
        if (m > n) return fa_fail(fc, GK_E_STATE, "gk_fasta_check: more codes than characters (internal error)");
        FA_HIP(fc, kt.start());
        hipLaunchKernelGGL((k_fa_squeeze<1>), dim3((unsigned)ntiles), dim3(FQ_BLOCK), 0, ctx->stream, T, n, slice_off, E, tile_off, fc->per_line, fc->d_st,
                           nullptr, kept_off, codes + FA_HEAD, src);
        if (terms) hipLaunchKernelGGL(k_fa_short, dim3((unsigned)((terms + FQ_BLOCK - 1) / FQ_BLOCK)), dim3(FQ_BLOCK), 0, ctx->stream, T, n, E, terms, k, fc->d_st);
        FA_HIP(fc, hipGetLastError());
        if ((rc = kt.end(&parse_ms))) { fc->failed = true; return rc; }
        // ---- windows
        const u32 nc = fc->nc;
        const u64 Ltot = nc + m, P = Ltot >= (u64)k ? Ltot - k + 1 : 0;
        const u64 nF = (P + 63) / 64, nC = (Ltot + 63) / 64, nshort = nF * 4;
        const u32 nc_new = (u32)std::min<u64>((u64)k - 1, Ltot);
        FaSlice sl{T, n, slice_off, E, terms, codes + FA_HEAD - nc, Ltot, P, src};
        const u64 w_before = fc->h[5], f_before = fc->h[6];
        FA_HIP(fc, kt.start());
        if (nc) hipLaunchKernelGGL(k_fa_put_carry, dim3(1), dim3(64), 0, ctx->stream, fc->d_st, codes, nc);
        if (P) {
            const unsigned grid = (unsigned)((nshort + 255) / 256);
            GK_BY_W(fc->W, hipLaunchKernelGGL(k_fa_windows<W>, dim3(grid), dim3(256), 0, ctx->stream, Table<W>{(Slot<W> *)slots, nb2, lnb1, k == 64 ? 1u : 0u, 0u}, k, sl.S,
                                              Ltot, P, (uint16_t *)wb, (uint16_t *)fb, nshort, fc->d_st));
        }
        if (nC) hipLaunchKernelGGL(k_fa_cover, dim3((unsigned)std::min<u64>((nC + 255) / 256, 4096)), dim3(256), 0, ctx->stream, fb, nF, nC, P, k, cb, fc->d_st);
        FA_HIP(fc, hipGetLastError());
        FA_HIP(fc, hipMemcpyAsync(fc->h, fc->d_st, FA_STATE_HOST, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = kt.end(&look_ms))) { fc->failed = true; return rc; }
        // ---- the first not-found windows, in stream order
        const u64 miss_now = (fc->h[5] - w_before) - (fc->h[6] - f_before);
        u64 appended = 0;
        if (want_pos && miss_now && fc->have < fc->max_missing) {
            appended = std::min<u64>(miss_now, fc->max_missing - fc->have);
            if ((rc = fa_miss_reserve(fc, fc->have + appended))) return rc;
            FA_HIP(fc, kt.start());
            const unsigned grid = (unsigned)std::min<u64>((nF + 255) / 256, 4096);
            hipLaunchKernelGGL(k_fa_miss_count, dim3(grid), dim3(256), 0, ctx->stream, wb, fb, nF, mcnt);
            FA_HIP(fc, hipGetLastError());
            FA_HIP(fc, scan_counts(ctx, mcnt, nF, moff, scan));
            const u64 mc = fc->miss_cap;
            hipLaunchKernelGGL(k_fa_miss_emit, dim3(grid), dim3(256), 0, ctx->stream, sl, fc->d_st, nc, k, wb, fb, nF, moff, fc->have, fc->max_missing, fc->d_miss,
                               fc->d_miss + mc, fc->d_miss + 2 * mc, fc->d_miss + 3 * mc, fc->d_miss + 4 * mc);
            FA_HIP(fc, hipGetLastError());
            if ((rc = kt.end(&look_ms))) { fc->failed = true; return rc; }
        }
        FA_HIP(fc, kt.start());
        hipLaunchKernelGGL(k_fa_carry, dim3(1), dim3(64), 0, ctx->stream, sl, fc->d_st, nc, nc_new, cb, appended);
        FA_HIP(fc, hipGetLastError());
        if ((rc = kt.end(&look_ms))) { fc->failed = true; return rc; }
        fc->nc = nc_new;
        fc->have += appended;
        if (!eblk) tmp.release(E);
        uploaded = next.len != 0;
        cut = next;
        b = 1 - b;
    }
    FA_HIP(fc, hipStreamSynchronize(ctx->copy_stream));
    fc->text_off += nbytes;
    fc->prev_cr = text[nbytes - 1] == '\r';
    fc->ms[0] = (float)up_ms; fc->ms[1] = (float)parse_ms; fc->ms[2] = (float)look_ms;
    return GK_OK;
}

}  // namespace

extern "C" {

int gk_fasta_check_create(gk_ctx *ctx, gk_vmap *positions, int per_line, uint64_t max_missing, gk_fasta_check **out) {
    if (!ctx || !out) return fail(ctx, GK_E_INVALID, "gk_fasta_check_create: null argument");
    *out = nullptr;
    if (!positions) return fail(ctx, GK_E_INVALID, "gk_fasta_check_create: null position map");
    if (vmap_ctx(positions) != ctx) return fail(ctx, GK_E_INVALID, "gk_fasta_check_create: the position map lives on another context");
    GK_HIP(ctx, hipSetDevice(ctx->device));
    gk_fasta_check *fc = new gk_fasta_check;
    fc->ctx = ctx; fc->vm = positions; fc->k = vmap_k(positions); fc->W = words_for_k(fc->k);
    fc->per_line = per_line ? 1 : 0; fc->max_missing = max_missing;
    hipError_t e = fc->up.create();
    if (e == hipSuccess) e = pool_malloc(ctx, &fc->d_st, sizeof(FaState));
    if (e == hipSuccess) e = hipHostMalloc((void **)&fc->h, 16 * 8, 0);
    if (e == hipSuccess) {
        FaState init{};
        init.first_hdr = init.first_seq = FA_NONE;
        memset(fc->h, 0, 16 * 8);
        fc->h[9] = fc->h[10] = FA_NONE;
        e = hipMemcpyAsync(fc->d_st, &init, sizeof(FaState), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) { const int rc = hip_fail(ctx, e, "gk_fasta_check_create"); gk_fasta_check_destroy(fc); return rc; }
    *out = fc;
    return GK_OK;
}

void gk_fasta_check_destroy(gk_fasta_check *fc) {
    if (!fc) return;
    gk_ctx *ctx = fc->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->copy_stream);
    (void)hipStreamSynchronize(ctx->stream);
    (void)pool_free(ctx, fc->d_st);
    (void)pool_free(ctx, fc->d_miss);
    fc->up.destroy();
    if (fc->h) (void)hipHostFree(fc->h);
    delete fc;
}

int gk_fasta_check_feed(gk_fasta_check *fc, const char *text, size_t nbytes, int last) {
    if (!fc) return fail(nullptr, GK_E_INVALID, "gk_fasta_check_feed: null handle");
    gk_ctx *ctx = fc->ctx;
    if (fc->failed) return fail(ctx, GK_E_STATE, "gk_fasta_check: the handle failed earlier (see the first error); destroy it");
    if (fc->finished) return fail(ctx, GK_E_STATE, "gk_fasta_check: the input has ended (last != 0 was passed)");
    if (!text && nbytes) return fail(ctx, GK_E_INVALID, "gk_fasta_check_feed: null text");
    GK_HIP(ctx, hipSetDevice(ctx->device));
    const auto t_call = clk::now();
    fc->ms[0] = fc->ms[1] = fc->ms[2] = 0;
    if (nbytes) { if (int rc = fa_run(fc, text, nbytes)) return rc; }
    if (last) {
        hipLaunchKernelGGL(k_fa_finish, dim3(1), dim3(1), 0, ctx->stream, fc->d_st, fc->k);
        FA_HIP(fc, hipGetLastError());
        fc->finished = true;
        fc->nc = 0;
    }
    FA_HIP(fc, read_back(ctx, {{fc->h, fc->d_st, FA_STATE_HOST}}));
    fc->ms[3] = (float)ms_since(t_call);
    return GK_OK;
}

int gk_fasta_check_stats(const gk_fasta_check *fc, uint64_t *lines, uint64_t *records, uint64_t *bases, uint64_t *valid_bases, uint64_t *windows,
                         uint64_t *found, uint64_t *missing, uint64_t *covered_bases, uint64_t *short_lines) {
    if (!fc) return fail(nullptr, GK_E_INVALID, "gk_fasta_check_stats: null handle");
    const unsigned long long *h = fc->h;
    if (lines) *lines = h[0] + h[1];
    if (records) *records = h[2] + (h[10] < h[9] ? 1 : 0);
    if (bases) *bases = h[3];
    if (valid_bases) *valid_bases = h[4];
    if (windows) *windows = h[5];
    if (found) *found = h[6];
    if (missing) *missing = h[5] - h[6];
    if (covered_bases) *covered_bases = h[7];
    if (short_lines) *short_lines = h[8];
    return GK_OK;
}

int gk_fasta_check_missing(const gk_fasta_check *fc, uint64_t *text_offset, uint64_t *line, uint64_t *column, uint64_t *lo, uint64_t *hi, uint64_t cap,
                           uint64_t *n) {
    if (!fc) return fail(nullptr, GK_E_INVALID, "gk_fasta_check_missing: null handle");
    gk_ctx *ctx = fc->ctx;
    if (n) *n = fc->have;
    const u64 take = std::min<u64>(fc->have, cap);
    if (!take) return GK_OK;
    GK_HIP(ctx, hipSetDevice(ctx->device));
    const unsigned long long *d = fc->d_miss;
    const u64 mc = fc->miss_cap, nb = take * 8;
    GK_HIP(ctx, read_back(ctx, {{text_offset, d, nb}, {line, d + mc, nb}, {column, d + 2 * mc, nb}, {lo, d + 3 * mc, nb}, {hi, d + 4 * mc, nb}}));
    return GK_OK;
}

int gk_fasta_check_last_ms(const gk_fasta_check *fc, float *ms4) {
    if (!fc) return fail(nullptr, GK_E_INVALID, "gk_fasta_check_last_ms: null handle");
    if (!ms4) return fail(fc->ctx, GK_E_INVALID, "gk_fasta_check_last_ms: null buffer");
    for (int i = 0; i < 4; i++) ms4[i] = fc->ms[i];
    return GK_OK;
}

}  // extern "C"

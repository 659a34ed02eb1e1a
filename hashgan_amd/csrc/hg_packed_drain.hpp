// hashgan_amd -- the batched drain of the packed matrix-core selects k_select_mx3 (hg_select_mx3.hpp, codes of <= 64
// bits) and k_select_mx4 (hg_select_mx4.hpp, 65..128 bits), and the block geometry the two kernels share.
//
// Both kernels harvest, per supertile (P::ROWS consecutive rows of a segment) and query tile, P::WORDS hit words per
// lane.  What differs between them -- rows per supertile, words per entry, the entry's size in the queue, how the words
// become a flat hit mask of the supertile -- is the kernel's traits struct P (M3Pack / M4Pack, next to m3_row / m4_row
// in the kernel's own header, with the entry format).  Everything else is here, once.
//
// Drain (one-byte compact records only: hg_mx_drain.hpp explains rings and slices).  Per supertile and query tile every
// lane with a hit appends ONE entry {A | query tag | row index of the supertile, B | slice position & 15, further
// words} to the wavefront's queue (ring buffer in LDS, slot = rank among the pushing lanes).  The emit works the queue
// off in batches of exactly 64 entries -- every lane busy -- and entries that do not fill a batch WAIT for the next
// window: the packed codes and labels the emit needs are triple-buffered, so an entry may be emitted one window late,
// and the owner-side flush of the 16-record rings lags one window accordingly (it flushes what was pushed before the
// window that just ended).  A block is P::WPB (eight) wavefronts = one segment pair x 512 queries sharing windows of
// P::ws(LW) supertiles; ~140 entries per window and wavefront at C2.
// Bursts (a ring that could overflow: > 16 records of one slice pending) drain everything and, if one supertile alone
// still brings too many, the lane walks its own hits straight to global memory -- rare, slow, exact.
//
// The traits of a packing:
//     QT, ROWS, WPB      query tiles (of 32) per wavefront, rows per supertile and lane-half, wavefronts per block
//     WORDS, ENTRY       hit words per entry, bytes of an entry in the LDS queue
//     CHUNKS, IMG_WORDS  1 KiB chunks of A fragments per supertile; 16-byte code words per row of the database image
//     ws(LW), WS_MAX     supertiles per window for LW label words (1, 2 or 4: the row index of a queue entry has five bits); the largest
//     FLUSH              the owners flush their rings every this many supertiles (a multiple of the window)
//     load / store       a queue entry <-> its words; OPAQUE_QBASE: the queue's LDS address is hidden from the optimiser
//     flat(words)        the supertile's hit mask, bit P <-> row P (the direct route)
//     Mask               the same for the emit's walk over an entry: any(), pop() = the earliest row left
#pragma once
#include "hg_select_mx.hpp"

namespace hg {

constexpr int PK_QCAP = 128;               // queue entries per wavefront (ring buffer; a power of two)
constexpr int PK_RING = 16;                // records per slice ring

// (x & K) | y in one op
__device__ __forceinline__ u32 pk_and_or(const u32 x, const u32 k, const u32 y) {
    u32 d;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(d) : "v"(x), "n"(k), "v"(y));
    return d;
}

// (x << SH) | y and a | b | c in one op each, c wave-uniform: a queue entry's two tagged words cost the push one op apiece
template <int SH> __device__ __forceinline__ u32 pk_lshl_or(const u32 x, const u32 y) {
    u32 d;
    asm("v_lshl_or_b32 %0, %1, %2, %3" : "=v"(d) : "v"(x), "n"(SH), "v"(y));
    return d;
}
__device__ __forceinline__ u32 pk_or3_s(const u32 a, const u32 b, const u32 c) {
    u32 d;
    asm("v_or3_b32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c));
    return d;
}

struct PackedLds {             // byte offsets inside the block's dynamic LDS
    int a, abuf;               // A fragments: 2 buffers of abuf bytes
    int cl, labels;            // packed codes of the staged rows, one array [3 buffers][2 lane-halves][window rows]; their labels, a second array indexed alike
    int qcodes, qlabels;       // the block's query tables
    int queue;                 // per-wave queues: [PK_QCAP] entries of P::ENTRY bytes
    int rings;                 // per-wave slice rings
    int total;
};
template <class P> __host__ __device__ inline PackedLds packed_lds_layout(int NW, int LW) {
    PackedLds l;
    const int WS = P::ws(LW), WROWS = WS * P::ROWS;
    l.a = 0;
    l.abuf = WS * P::CHUNKS * 1024;
    l.cl = 2 * l.abuf;
    l.labels = l.cl + 6 * WROWS * NW * 4;
    l.qcodes = (l.labels + 6 * WROWS * LW * 8 + 15) & ~15;
    l.qlabels = l.qcodes + P::WPB * 64 * NW * 4;
    l.queue = l.qlabels + P::WPB * 64 * LW * 8;
    l.rings = l.queue + P::WPB * PK_QCAP * P::ENTRY;
    l.total = l.rings + P::WPB * 64 * P::QT * PK_RING;
    return l;
}

template <int NW, int LW, class P>
struct PackedDrain {
    static constexpr int QT = P::QT, NH = P::WORDS, CB = NW * 4, LB = LW * 8;
    static constexpr int ROWS = P::ROWS, WROWS = P::ws(LW) * ROWS;
    static_assert((P::ws(LW) & (P::ws(LW) - 1)) == 0 && 6 * P::ws(LW) <= 32, "an entry's row index: {buffer, lane-half, supertile} in five bits, the half one of them");
    u8* lds;
    PackedLds L;
    u32 ring_base;                       // LDS address of the wavefront's first ring
    u32 qbase;                           // this wavefront's queue: LDS address of its first entry (kept opaque: ONE address per entry)
    u8* rings;                           // this wavefront's rings: slice (t, lane) at ring_index(t) * PK_RING
    int wave, lane;
    u32 cap;                             // slice capacity (records), a multiple of 16
    u8* tb0;                             // the wavefront's first slice (t = 0, lane 0); tile t adds t * 32 * crow
    i64 crow;
    u32 lane_off;                        // byte offset of the lane's slices relative to that (the launcher keeps 64 * crow below 2^31)
    u32 cnt[QT];                         // records of slice (t, lane) pushed so far (may exceed cap: the surplus is dropped at the flush)
    u32 prev[QT];                        // ... pushed before the current window: those are in the rings for sure
    u32 flushed[QT];                     // ... written to global memory (a multiple of 8)
    u32 qhead, qfill, old;               // queue: first entry, entries, entries pushed before the current window (wave-uniform)
    int probe;

    __device__ __forceinline__ void init(u8* lds_, const PackedLds& L_, int wave_, int lane_, int qb, int sp, u32 cap_, i64 crow_, u8* cand8, int probe_) {
        lds = lds_; L = L_; wave = wave_; lane = lane_; cap = cap_; crow = crow_; probe = probe_;
        qbase = (u32)(L.queue + wave * (PK_QCAP * P::ENTRY));
        if (P::OPAQUE_QBASE) asm volatile("" : "+s"(qbase));
        rings = lds + L.rings + wave * (64 * QT * PK_RING);
        ring_base = (u32)(uintptr_t)(__attribute__((address_space(3))) u8*)rings;
        const int h = lane >> 5, j = lane & 31;
        lane_off = (u32)j * (u32)crow + (u32)h * cap;
        tb0 = cand8 + (i64)(qb * P::WPB + wave) * 64 * crow + (i64)(2 * sp) * cap;
        qhead = qfill = old = 0;
#pragma unroll
        for (int t = 0; t < QT; ++t) cnt[t] = prev[t] = flushed[t] = 0;
    }
    // ring of slice (t, lane): half * 64 + t * 32 + query-in-tile -- the low six bits are the tag a queue entry carries
    __device__ __forceinline__ int ring_index(const int t) const { return (lane >> 5) * 64 + t * 32 + (lane & 31); }
    __device__ __forceinline__ u8* slice(const int t) const { return tb0 + (i64)t * 32 * crow + lane_off; }
    // n + the hits of one query tile's words (summed in this order: cnt + pop(A) + pop(B) + ...)
    static __device__ __forceinline__ u32 plus_hits(u32 n, const u32 (&w)[NH]) {
#pragma unroll
        for (int k = 0; k < NH; ++k) n += (u32)__builtin_popcount(w[k]);
        return n;
    }

    // ---- owner side: completed 8-record pieces below limit[t] leave the ring with one aligned 8-byte store each ----
    // (a slice that is already full keeps advancing: its surplus pieces land on its last piece -- the query is flagged
    // as lost at the end of the kernel, what its slice holds no longer matters, only that the stores stay inside it)
    __device__ __forceinline__ void flush_to(const u32 (&limit)[QT]) {
        bool need = false;
#pragma unroll
        for (int t = 0; t < QT; ++t) need |= limit[t] - flushed[t] >= 8u;
        while (__any(need)) {                                         // a second pass only if some slice had 16 pending
            need = false;
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                const u32 f = flushed[t];
                if (limit[t] - f >= 8u) {
                    const u8* ring = rings + ring_index(t) * PK_RING;
                    u8* tb = tb0 + (i64)t * 32 * crow;                // wave-uniform base; the lane's part fits 32 bits
                    *(u64*)(tb + (lane_off + min(f, cap - 8u))) = *(const u64*)(ring + (f & 8u));
                    flushed[t] = f + 8u;
                    need |= limit[t] - f >= 16u;
                }
            }
        }
        wave_lds_sync();                                              // ring reads done before an emit reuses the slots
    }

    // ---- emit: n <= 64 entries from the head of the queue, one per lane ----
    __device__ __forceinline__ void emit_batch(const u32 n) {
        wave_lds_sync();
        if ((u32)lane < n && !(kProbes && (probe & 8))) {
            const u32 i = (qhead + (u32)lane) & (PK_QCAP - 1);
            u32 e[NH];
            P::load(lds, qbase, i, e);
            // every packing's entry: e[0] = {query tag t * 32 + j : 6 | hit bits | idx : 5}, e[1] = {hit bits | position : 5};
            // idx = (buffer * 2 + lane-half) * WS + supertile numbers the supertile's rows among the staged ones, codes and labels alike
            const u32 x = e[0] & 63u, idx = e[0] >> 27, h = (idx / (u32)P::ws(LW)) & 1u;
            u32 pos = e[1] >> 27;                                     // slice position & 15 of the entry's first hit
            typename P::Mask m(e);
            const u32 ql = (u32)wave * 64u + x;                       // the entry's query, block-local
            u32 qcw[NW];
            u64 qlw[LW];
            // (plain LDS addresses -- the block's dynamic LDS starts at 0 -- spare the add of the array's symbol)
#pragma unroll
            for (int k = 0; k < NW; ++k) qcw[k] = ((const u32 __attribute__((address_space(3)))*)(uintptr_t)((u32)L.qcodes + ql * CB))[k];
#pragma unroll
            for (int k = 0; k < LW; ++k) qlw[k] = ((const u64 __attribute__((address_space(3)))*)(uintptr_t)((u32)L.qlabels + ql * LB))[k];
            const u32 ring = ring_base + (h * 64u + x) * PK_RING;     // LDS address (the block's dynamic LDS starts at 0), a multiple of 16
            // LDS byte offsets of the code / label words of the supertile's row 0
            const u32 code0 = (u32)L.cl + idx * (u32)(ROWS * CB);
            const u32 lab0 = (u32)L.labels + idx * (u32)(ROWS * LB);
            while (m.any()) {
                const u32 row = m.pop();                              // lowest set bit = earliest row
                const u32* rp = (const u32*)(lds + (code0 + row * CB));
                u32 d = 0;
#pragma unroll
                for (int k = 0; k < NW; ++k) d += __builtin_popcount(qcw[k] ^ rp[k]);
                const u64* lp = (const u64*)(lds + (lab0 + row * LB));
                u64 any = 0;
#pragma unroll
                for (int k = 0; k < LW; ++k) any |= lp[k] & qlw[k];
                if (!(kProbes && (probe & 4))) *(u8 __attribute__((address_space(3)))*)(uintptr_t)pk_and_or(pos, PK_RING - 1, ring) = make_rec8(d, any != 0);
                ++pos;
            }
        }
        wave_lds_sync();
        qhead = (qhead + n) & (PK_QCAP - 1);
        qfill -= n;
        old = old > n ? old - n : 0u;
    }
    __device__ __forceinline__ void emit_all() {
        while (qfill) emit_batch(qfill < 64u ? qfill : 64u);
    }

    // ---- rare: the lane writes the hits of one of its own supertile masks straight to global memory ----
    // (its ring's leftovers first, so the slice stays in index order; every record also passes through the ring, whose
    // last partial piece is then what a later flush expects)
    __device__ __forceinline__ void direct_walk(const int t, const u32 (&w)[NH], const int st, const u32 sel) {
        const u8* ring_r = rings + ring_index(t) * PK_RING;
        u8* ring = rings + ring_index(t) * PK_RING;
        u8* out = slice(t);
        for (u32 p = flushed[t]; p < cnt[t]; ++p) if (p < cap) out[p] = ring_r[p & (PK_RING - 1)];
        auto x = P::flat(w);                                          // u32 or u64, as the supertile has rows
        const int ql = wave * 64 + t * 32 + (lane & 31);
        u32 qcw[NW];
        u64 qlw[LW];
#pragma unroll
        for (int k = 0; k < NW; ++k) qcw[k] = ((const u32*)(lds + L.qcodes + ql * CB))[k];
#pragma unroll
        for (int k = 0; k < LW; ++k) qlw[k] = ((const u64*)(lds + L.qlabels + ql * LB))[k];
        const u32 row0 = (sel * 2u + (u32)(lane >> 5)) * WROWS + (u32)st * ROWS;
        const u8* codes = lds + L.cl;
        const u8* labels = lds + L.labels;
        u32 pos = cnt[t];
        while (x) {
            const u32 row = (u32)(sizeof(x) == 8 ? __builtin_ctzll(x) : __builtin_ctz((u32)x));
            x &= x - 1;
            const u32* rp = (const u32*)(codes + (row0 + row) * CB);
            u32 d = 0;
#pragma unroll
            for (int k = 0; k < NW; ++k) d += __builtin_popcount(qcw[k] ^ rp[k]);
            const u64* lp = (const u64*)(labels + (row0 + row) * LB);
            u64 any = 0;
#pragma unroll
            for (int k = 0; k < LW; ++k) any |= lp[k] & qlw[k];
            const u8 rec = make_rec8(d, any != 0);
            if (pos < cap) out[pos] = rec;
            ring[pos & (PK_RING - 1)] = rec;
            ++pos;
        }
        cnt[t] = pos;
        prev[t] = pos;
        flushed[t] = pos & ~7u;
    }

    // Rare: the queue cannot take this supertile's entries, or some slice would have more than PK_RING unflushed records.
    // Everything queued is emitted and flushed; slices that still cannot take their hits go the direct route and their
    // words are cleared.
    __device__ __forceinline__ void make_room(u32 (&w)[QT][NH], const int st, const u32 sel) {
        emit_all();
#pragma unroll
        for (int t = 0; t < QT; ++t) prev[t] = cnt[t];
        flush_to(prev);
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const u32 want = plus_hits(cnt[t], w[t]);
            if (want - flushed[t] > (u32)PK_RING) {
                direct_walk(t, w[t], st, sel);
#pragma unroll
                for (int k = 0; k < NH; ++k) w[t][k] = 0u;
            }
        }
        wave_lds_sync();
    }

    // The hit words of one supertile: w[t] = the words of query tile t.  st = supertile of the window, sel = the
    // window's codes/labels buffer.
    __device__ __forceinline__ void push(u32 (&w)[QT][NH], const int st, const u32 sel) {
        u32 want[QT];
        u64 bal[QT];
        {
            bool over = false;
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                want[t] = plus_hits(cnt[t], w[t]);
                over |= want[t] - flushed[t] > (u32)PK_RING;
            }
            if (__builtin_expect(__any(over) != 0, 0)) {              // rare: afterwards every ring takes what is left of the words
                make_room(w, st, sel);
#pragma unroll
                for (int t = 0; t < QT; ++t) want[t] = plus_hits(cnt[t], w[t]);
            }
        }
        // (a lane has a hit where its count moves -- the popcounts are needed anyway; ONE definition, behind the rare branch: no second
        // compare for the stores' exec mask)
#pragma unroll
        for (int t = 0; t < QT; ++t) bal[t] = __ballot(want[t] != cnt[t]);
        u32 nz = 0;
#pragma unroll
        for (int t = 0; t < QT; ++t) nz += (u32)__builtin_popcountll(bal[t]);
        if (__builtin_expect(qfill + nz > (u32)PK_QCAP, 0)) {         // a full queue: work off whole batches (never wasted work);
            while (qfill >= 64u) emit_batch(64u);                     // a dense supertile (up to 128 entries) needs it empty
            if (qfill + nz > (u32)PK_QCAP) emit_batch(qfill);
        }
        // the entry's row index (buffer * 2 + half) * WS + supertile: the wave-uniform part is scalar, the half's rides in the lane's constant
        const u32 desc = (sel * (u32)(2 * P::ws(LW)) + (u32)st) << 27;
        const u32 half = (u32)(lane >> 5) * (u32)P::ws(LW);
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const u64 b = bal[t];
            const u32 slot = (qhead + qfill + __builtin_amdgcn_mbcnt_hi((u32)(b >> 32), __builtin_amdgcn_mbcnt_lo((u32)b, 0u))) & (PK_QCAP - 1);
            if (__builtin_amdgcn_inverse_ballot_w64(b)) {             // (the ballot IS the exec mask: no second compare)
                u32 e[NH];
                // (the lane's part is the same for every tile; the tile's bit joins the scalar part)
                e[0] = pk_or3_s(w[t][0], (u32)(lane & 31) | (half << 27), desc | ((u32)t << 5));
                e[1] = pk_lshl_or<27>(cnt[t], w[t][1]);
#pragma unroll
                for (int k = 2; k < NH; ++k) e[k] = w[t][k];
                P::store(lds, qbase, slot, e);
            }
            cnt[t] = want[t];
            qfill += (u32)__builtin_popcountll(b);
        }
    }

    // End of a window: entries pushed before it must be emitted now (their codes/labels buffer is recycled next); of
    // this window's, whole batches only.  Then the owners flush what was pushed before this window.
    __device__ __forceinline__ void end_window(const bool do_flush) {
        while (qfill >= 64u) emit_batch(64u);
        if (old) emit_batch(qfill);
        old = qfill;
        if (do_flush) flush_to(prev);
#pragma unroll
        for (int t = 0; t < QT; ++t) prev[t] = cnt[t];
    }

    // End of the kernel: everything out; the last partial piece of a slice leaves as a whole 8-byte store (slots past
    // cnt are inside the slice's capacity, a multiple of 16).
    __device__ __forceinline__ void finish() {
        emit_all();
        flush_to(cnt);
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const u32 f = flushed[t];
            if (cnt[t] > f) {
                const u8* ring = rings + ring_index(t) * PK_RING;
                *(u64*)(slice(t) + min(f, cap - 8u)) = *(const u64*)(ring + (f & 8u));
            }
        }
    }
};

// ---- the block's place in the database, the same in both kernels ----
// Geo as set by the launcher: g.nQT = query blocks (of 64 P::WPB queries) per segment pair, g.nBlk = blocks; g.L % P::ROWS == 0.
// Logical block lb = one pair of segments x one block of queries; lane-half h of every wavefront works on segment 2 sp + h.
template <int LW, class P>
struct PackedBlock {
    int sp, qb;                          // segment pair, block of 64 P::WPB (512) queries
    int h, j;                            // lane-half, lane of the half
    int s;                               // this lane's segment
    bool seg_ok;
    i64 lo0, lo1, len0, len1;            // first row and length of the pair's two segments
    i64 mylen, minlen;                   // length of this lane's segment; of the shorter one
    i64 nwin;                            // windows of the longer one: both walk that many
    i64 NG;                              // supertiles in the image

    __device__ __forceinline__ PackedBlock(const int lb, const int lane, const Geo& g) {
        constexpr int WROWS = P::ws(LW) * P::ROWS;
        const int nQB = g.nQT;
        sp = lb / nQB;
        qb = lb - sp * nQB;
        h = lane >> 5; j = lane & 31;
        s = 2 * sp + h;
        seg_ok = s < g.S;
        lo0 = (i64)(2 * sp) * g.L; lo1 = lo0 + g.L;
        len0 = (lo0 + g.L < g.N ? g.L : g.N - lo0);
        len1 = lo1 >= g.N ? 0 : (lo1 + g.L < g.N ? g.L : g.N - lo1);
        mylen = h ? len1 : len0;
        minlen = len0 < len1 ? len0 : len1;
        nwin = ((len0 > len1 ? len0 : len1) + WROWS - 1) / WROWS;
        NG = (g.N + P::ROWS - 1) / P::ROWS;
    }
};

}  // namespace hg

// revcomp_kernel.hip -- reverseComplement.c:21-118 as data-parallel byte
// kernels (HBM-bound map + scans).  Included by imsame_dev.hip.
//
// Semantics restated:
//  * every '>' byte opens a record (:48-54); records are emitted last first (:56)
//  * header = bytes from the '>' through the first '\n' (fgets, :59-62)
//  * body   = bytes after the header up to the next '>' (:64-70); only
//    letters (isupper || islower) are kept, reversed, complemented
//    A<->T C<->G U->A, case kept, other letters unchanged (:71-106)
//  * one '\n' after each record's sequence (:109-110)
// Records whose '>' sits inside another header share that header's body (and
// repeat the rest of that header), so an image's output can be far larger
// than the image: positions inside an image are u32 (an image is below
// 4 GiB - 16), output offsets are u64.
//
// No thread's trip count grows with the length of a line: header ends come
// from the newline ranks (rc_scan: the rank of the first '\n' at or after each
// '>', and the compacted newline positions), headers are copied per byte.
// The one loop left (rc_write) runs once per output byte it writes.

__device__ __forceinline__ bool rc_is_letter(uint8_t c) { return (uint8_t)((c | 0x20) - 'a') < 26u; }

__device__ __forceinline__ uint8_t rc_comp(uint8_t c) {
    switch (c) {
    case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; case 'U': return 'A';
    case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a'; case 'u': return 'a';
    }
    return c;
}

// A block takes RC_TILE bytes, 16 per thread (one 16-byte load; the image
// buffer is padded so the last load stays inside it, bytes at >= n count as
// nothing).  The three per-thread counts ('>', letters, '\n': <= 16 each,
// <= 4096 per block) travel packed in one u64, 21 bits each.
#define RC_THREADS 256
#define RC_TILE (RC_THREADS * 16)
#define RC_SH 21
#define RC_MASK ((1u << RC_SH) - 1)

__device__ __forceinline__ uint64_t rc_count16(const uint8_t *in, uint64_t n, uint64_t b, uint8_t *c16) {
    uint64_t pk = 0;
    if (b < n) {
        *(uint4 *)c16 = *(const uint4 *)(in + b);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint8_t c = b + k < n ? c16[k] : (uint8_t)0;
            c16[k] = c;
            pk += (uint64_t)(c == '>') | ((uint64_t)rc_is_letter(c) << RC_SH) | ((uint64_t)(c == '\n') << (2 * RC_SH));
        }
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) c16[k] = 0;
    }
    return pk;
}

// pass 1: per-tile totals of '>', letters and newlines
__global__ void __launch_bounds__(RC_THREADS) rc_count(const uint8_t *in, uint64_t n, uint32_t *bgt, uint32_t *blet,
                                                        uint32_t *bnl) {
    __shared__ unsigned long long acc;
    if (threadIdx.x == 0) acc = 0;
    __syncthreads();
    alignas(16) uint8_t c16[16];
    const uint64_t pk = rc_count16(in, n, (blockIdx.x * (uint64_t)RC_THREADS + threadIdx.x) * 16, c16);
    if (pk) atomicAdd(&acc, (unsigned long long)pk);
    __syncthreads();
    if (threadIdx.x == 0) {
        bgt[blockIdx.x] = (uint32_t)(acc & RC_MASK);
        blet[blockIdx.x] = (uint32_t)((acc >> RC_SH) & RC_MASK);
        bnl[blockIdx.x] = (uint32_t)((acc >> (2 * RC_SH)) & RC_MASK);
    }
}

// pass 2, with the scanned tile totals: gpos[i] / let[i] = '>' / letters
// before byte i, for i in [0, n] (the arrays hold n + 32 entries: every
// thread with b <= n stores its 16); off[] record starts, rnl[] the newline
// rank at each record's start, nlpos[] the newline positions.
__global__ void __launch_bounds__(RC_THREADS) rc_scan(const uint8_t *in, uint64_t n, const uint32_t *pgt,
                                                       const uint32_t *plet, const uint32_t *pnl, uint32_t *gpos,
                                                       uint32_t *let, uint32_t *off, uint32_t *rnl, uint32_t *nlpos) {
    __shared__ uint64_t s[RC_THREADS];
    const uint32_t t = threadIdx.x;
    const uint64_t b = (blockIdx.x * (uint64_t)RC_THREADS + t) * 16;
    alignas(16) uint8_t c16[16];
    const uint64_t pk = rc_count16(in, n, b, c16);
    s[t] = pk;
    __syncthreads();
    for (uint32_t o = 1; o < RC_THREADS; o <<= 1) {
        const uint64_t v = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    if (b > n) return;
    const uint64_t ex = s[t] - pk;
    uint32_t g = pgt[blockIdx.x] + (uint32_t)(ex & RC_MASK);
    uint32_t l = plet[blockIdx.x] + (uint32_t)((ex >> RC_SH) & RC_MASK);
    uint32_t r = pnl[blockIdx.x] + (uint32_t)((ex >> (2 * RC_SH)) & RC_MASK);
    alignas(16) uint32_t og[16], ol[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint8_t c = c16[k];
        og[k] = g; ol[k] = l;
        if (c == '>') { off[g] = (uint32_t)(b + k); rnl[g] = r; ++g; }
        else if (c == '\n') nlpos[r++] = (uint32_t)(b + k);
        else l += rc_is_letter(c);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ((uint4 *)(gpos + b))[k] = ((const uint4 *)og)[k];
        ((uint4 *)(let + b))[k] = ((const uint4 *)ol)[k];
    }
}

// per record k: header end (exclusive, after '\n'), body end, output size
// (in reverse record order, szr[nr] = 0 for the scan's total)
__global__ void rc_records(uint64_t n, const uint32_t *off, const uint32_t *rnl, const uint32_t *nlpos, uint32_t nnl,
                           uint32_t nr, const uint32_t *gpos, const uint32_t *let, uint32_t *hend, uint32_t *bend,
                           uint32_t *szr) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) szr[nr] = 0;
    if (k >= nr) return;
    const uint32_t r = rnl[k];
    const uint32_t h = r < nnl ? nlpos[r] + 1 : (uint32_t)n;
    const uint32_t nx = gpos[h];               // first record that starts at or after h
    const uint32_t b = nx < nr ? off[nx] : (uint32_t)n;
    hend[k] = h;
    bend[k] = b;
    szr[nr - 1 - k] = (h - off[k]) + (let[b] - let[h]) + 1;
}

// Every byte at or after the first '>' goes to each record that holds it: a
// header byte to the records whose '>' precedes it on its line, a body letter
// (reversed, complemented) to the records of the line that ends at its
// body's start.  Those records are consecutive and share hend.  The thread of
// a record's '>' also writes the record's closing '\n'.
__global__ void rc_write(const uint8_t *in, uint64_t n, const uint32_t *off, uint32_t nr, const uint32_t *hend,
                         const uint32_t *gpos, const uint32_t *let, const uint64_t *oo, uint8_t *out) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t cnt = gpos[i + 1];          // records that start at or before i
    if (cnt == 0) return;
    const uint8_t c = in[i];
    const uint32_t j = cnt - 1, h = hend[j];
    if (i < h) {
        for (int64_t k = j; k >= 0 && hend[k] == h; --k) out[oo[nr - 1 - k] + (i - off[k])] = c;
        if (c == '>') out[oo[nr - j] - 1] = '\n';          // record j's output ends where the next begins
        return;
    }
    if (!rc_is_letter(c)) return;
    const uint8_t v = rc_comp(c);
    const uint32_t back = let[i] - let[h] + 1;  // this letter's place from the end of the sequence
    for (int64_t k = j; k >= 0 && hend[k] == h; --k) out[oo[nr - k] - 1 - back] = v;
}

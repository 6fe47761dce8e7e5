// elf_device.inc -- ExtendLoopFast with its block table on the device
// (SURVEY.md §8 f2; included by block_build.hip before extend_loop_fast).
//
// The host loop (extend_loop_fast) keeps the blocks on the host and, every
// iteration, downloads FixEnds' results to slice the blocks, runs
// OverlaplessUnion, block_hash and MoveUnchanged over host blocks and builds
// the next flank batch.  Here the blocks live in a device table (DBlk /
// DFrag, double-buffered) for the whole loop and every one of those steps is
// a kernel:
//   block_hash (block_hash.cpp:29-55) over fragment ids formatted on the
//   device; MoveUnchanged (MoveUnchanged.cpp:37-67) as a device hash set;
//   the FragmentsExtender plan (FragmentsExtender.cpp:34-80) and the flank
//   decode; the stitch revcomp(left) + row + right (:108-118); FixEnds'
//   column jobs, kernels and slicing (FixEnds.cpp:117-144, Block::slice);
//   OverlaplessUnion (OverlaplessUnion.cpp:25-80: priority order by a merge
//   sort with the pinned tie-breaks, conflicts from one sort of every
//   fragment by sequence and start, greedy admission in priority sweeps);
//   the Pipe's state hash (Pipe.cpp:60-78).
// The host sees, per iteration, ONE summary download (the last iteration's
// state hash, OverlaplessUnion's fallback flag and the next batch's jobs --
// rows and flank length each, all the aligner's host planning needs) and the
// aligner's own result download.  OverlaplessUnion falls back to the host
// for inputs outside the device path's rules (a block overlapping itself, a
// fragment outside its sequence: SetFc's multiset mode), which the summary
// flags; the host then runs it on a downloaded table.

struct DBlk {
    int32_t fo, nf;     // first fragment, fragment count
    int32_t len, flags; // alignment length; DB_*
    uint64_t hash;      // block_hash (DB_HASH)
};
enum { DB_ROWS = 1, DB_HELD = 2, DB_HASH = 4 };
struct DFrag {
    int64_t min, max, roff;
    int32_t seq, ori;
};

// per iteration, device -> host (one copy)
struct ElfSum {
    uint64_t state;        // blockset hash of the table (blocks of more than one fragment)
    int64_t nb, nfr;       // table counts
    int64_t bytes;         // rows of the table: sum of pad16(nf * len) (the next stitch's source)
    int64_t nj, nrows;     // the planned batch: jobs, rows
    int64_t flank;         // ... flank residues
    int32_t max_len, max_sh;
    int32_t flags;         // ES_*
    int32_t pad;
    int64_t ou_in, ou_rej; // OverlaplessUnion of the last iteration
    int64_t fresh;         // MoveUnchanged: hashes added to the seen set
    int64_t n_small, n_large, n_tiles;  // FixEnds job lists (device-side launch counts)
    int64_t nb1, nfr1;     // the table after FixEnds' slicing (OverlaplessUnion's input)
    int32_t align_err;     // the aligner: a job overflowed its proven bound (AlignAsync::err)
    uint32_t align_epoch;  // ... its highest word-table epoch (AlignAsync::epoch)
    int64_t n_pieces;      // the stitch's copy pieces (StitchPass)
    uint32_t tickets[8];   // the single-launch table passes' tile tickets, one per pass kind
};
enum { ES_OU_HOST = 1, ES_FLANK_RANGE = 2, ES_LEN_RANGE = 4, ES_OU_CAP = 8 };

struct DJob {              // a planned flank job
    int32_t block, side, nf, sh;
    int64_t base;          // flank offset of its row 0 (rows at base + i * sh)
};
typedef JobRows DRes;      // the aligner's result of a job: row k at p + k * stride
struct DRow {              // a flank row to decode
    int64_t pos, dst;
    int32_t seq, ori, len, pad;
};

static constexpr int WG = 1024;  // single-workgroup table passes

// A block's fragments in batches of FB: the batch's loads issued together,
// then f(k, fragment) for each.  The table passes run one thread per block,
// and a loop that stores after each fragment load waits a memory round trip
// per fragment (the compiler cannot move a load above a store it may alias):
// ~17 of them a pass at C3.
template <int FB = 8, class F>
__device__ __forceinline__ void frag_batches(const DFrag* src, int n, F f) {
    for (int k0 = 0; k0 < n; k0 += FB) {
        DFrag fr[FB];
#pragma unroll
        for (int j = 0; j < FB; j++)
            if (k0 + j < n) fr[j] = src[k0 + j];
#pragma unroll
        for (int j = 0; j < FB; j++)
            if (k0 + j < n) f(k0 + j, fr[j]);
    }
}
// ... with a second load per fragment (pre(k, fragment)) issued with the batch
template <int FB = 8, class Pre, class F>
__device__ __forceinline__ void frag_batches_pre(const DFrag* src, int n, Pre pre, F f) {
    for (int k0 = 0; k0 < n; k0 += FB) {
        DFrag fr[FB];
        decltype(pre(0, fr[0])) px[FB];
#pragma unroll
        for (int j = 0; j < FB; j++)
            if (k0 + j < n) fr[j] = src[k0 + j];
#pragma unroll
        for (int j = 0; j < FB; j++)
            if (k0 + j < n) px[j] = pre(k0 + j, fr[j]);
#pragma unroll
        for (int j = 0; j < FB; j++)
            if (k0 + j < n) f(k0 + j, fr[j], px[j]);
    }
}

// Exclusive prefix sums over a single workgroup: thread t owns items
// [lo, hi); its per-item values are summed by the caller, handed here, and
// the thread gets its base (and every thread the total).
template <int K>
__device__ __forceinline__ void wg_scan(int64_t (&v)[K], int64_t (&tot)[K]) {
    __shared__ int64_t sh[K][WG];
    const int t = threadIdx.x;
    for (int k = 0; k < K; k++) sh[k][t] = v[k];
    __syncthreads();
    for (int off = 1; off < WG; off <<= 1) {
        int64_t add[K];
        for (int k = 0; k < K; k++) add[k] = t >= off ? sh[k][t - off] : 0;
        __syncthreads();
        for (int k = 0; k < K; k++) sh[k][t] += add[k];
        __syncthreads();
    }
    for (int k = 0; k < K; k++) {
        tot[k] = sh[k][WG - 1];
        v[k] = sh[k][t] - v[k];
    }
    __syncthreads();
}

__device__ __forceinline__ int64_t pad16d(int64_t x) { return (x + 15) & ~(int64_t)15; }

// ---- table passes: every pass over the table is "count per block, exclusive
// prefix sums, fill per block".  A pass P supplies n(), count(i, v) (adds its
// K values), fill(i, base, tot) (writes at base, advancing it) and
// totals(tot).  Small tables run in ONE workgroup (k_pass_wg: each thread a
// contiguous run of blocks, one wg_scan); large ones as one launch of
// 256-block tiles with decoupled look-back (k_pass_lb; run_pass on the host).
template <int K>
struct VK {
    int64_t v[K];
};
template <int K>
__host__ __device__ inline VK<K> operator+(const VK<K>& a, const VK<K>& b) {
    VK<K> r;
    for (int k = 0; k < K; k++) r.v[k] = a.v[k] + b.v[k];
    return r;
}
template <class P>
__global__ __launch_bounds__(WG) void k_pass_wg(P p) {
    if (p.skip()) return;
    constexpr int K = P::K;
    const int t = threadIdx.x;
    const int64_t n = p.n();
    const int64_t chunk = (n + WG - 1) / WG;
    const int64_t lo = min(n, chunk * t), hi = min(n, lo + chunk);
    int64_t v[K];
    for (int k = 0; k < K; k++) v[k] = 0;
    for (int64_t i = lo; i < hi; i++) p.count(i, v);
    int64_t tot[K];
    wg_scan<K>(v, tot);
    for (int64_t i = lo; i < hi; i++) p.fill(i, v, tot);
    if (t == 0) p.totals(tot);
}

// One launch for a whole pass (tables above the single-workgroup size):
// 256-block tiles take tickets in the order they start, count, scan their
// counts in LDS and find their prefix by decoupled look-back over the earlier
// tiles (each publishes its aggregate, then its inclusive prefix; a tile waits
// only on tiles that started before it), then fill.  Flags carry the launch's
// epoch, so they are never cleared.  The thread of the last block calls
// totals().  (The fills need no grand total: OuPrepPass's tie ranks above.)
struct LbState {
    uint32_t* flag;   // per tile: epoch << 2 | 1 (aggregate) / 2 (inclusive prefix)
    char* agg;        // per tile: VK<K>
    char* incl;       // per tile: VK<K>
};
template <class P>
__global__ __launch_bounds__(256) void k_pass_lb(P p, LbState L, uint32_t* __restrict__ ticket, uint32_t epoch) {
    constexpr int K = P::K;
    typedef VK<K> V;
    __shared__ int64_t sh[K][256];
    __shared__ uint32_t s_tile;
    __shared__ int64_t s_pre[K];
    if (p.skip()) return;
    const int tid = threadIdx.x;
    if (tid == 0) s_tile = atomicAdd(ticket, 1u);
    __syncthreads();
    const int64_t t = s_tile;
    const int64_t n = p.n();
    const int64_t i = t * 256 + tid;
    int64_t v[K];
    for (int k = 0; k < K; k++) v[k] = 0;
    if (i < n) p.count(i, v);
    // tile-wide exclusive scan
    for (int k = 0; k < K; k++) sh[k][tid] = v[k];
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        int64_t add[K];
        for (int k = 0; k < K; k++) add[k] = tid >= off ? sh[k][tid - off] : 0;
        __syncthreads();
        for (int k = 0; k < K; k++) sh[k][tid] += add[k];
        __syncthreads();
    }
    if (tid == 0) {
        V agg, pre;
        for (int k = 0; k < K; k++) {
            agg.v[k] = sh[k][255];
            pre.v[k] = 0;
        }
        V* A = (V*)L.agg;
        V* I = (V*)L.incl;
        const uint32_t ep = epoch & 0x3FFFFFFFu;
        if (t > 0) {
            A[t] = agg;
            __hip_atomic_store(&L.flag[t], (ep << 2) | 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            for (int64_t q = t - 1; q >= 0; q--) {
                uint32_t f;
                do {
                    f = __hip_atomic_load(&L.flag[q], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                } while ((f >> 2) != ep || (f & 3u) == 0);
                const V x = (f & 3u) == 2 ? I[q] : A[q];
                for (int k = 0; k < K; k++) pre.v[k] += x.v[k];
                if ((f & 3u) == 2) break;
            }
        }
        V inc;
        for (int k = 0; k < K; k++) inc.v[k] = pre.v[k] + agg.v[k];
        I[t] = inc;
        __hip_atomic_store(&L.flag[t], (ep << 2) | 2u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        for (int k = 0; k < K; k++) s_pre[k] = pre.v[k];
    }
    __syncthreads();
    int64_t base[K], tot[K];
    for (int k = 0; k < K; k++) {
        base[k] = s_pre[k] + sh[k][tid] - v[k];
        tot[k] = base[k] + v[k];
    }
    if (i < n) p.fill(i, base, tot);
    if (i == n - 1 || (n == 0 && i == 0)) p.totals(tot);  // (tot: the inclusive sum at the last block)
}

// ------------------------------------------------------------------ block_hash
__device__ int fmt_i64_d(char* p, int64_t x) {
    char t[24];
    int n = 24;
    const bool neg = x < 0;
    uint64_t u = neg ? (uint64_t)(-(x + 1)) + 1 : (uint64_t)x;
    do {
        t[--n] = (char)('0' + (int)(u % 10));
        u /= 10;
    } while (u);
    if (neg) t[--n] = '-';
    for (int i = n; i < 24; i++) p[i - n] = t[i];
    return 24 - n;
}

__device__ __forceinline__ int scmp_d(const char* a, int la, const char* b, int lb) {
    const int m = la < lb ? la : lb;
    for (int i = 0; i < m; i++) {
        const unsigned char x = (unsigned char)a[i], y = (unsigned char)b[i];
        if (x != y) return x < y ? -1 : 1;
    }
    return la < lb ? -1 : la > lb ? 1 : 0;
}

// block_hash_value (the host restatement above) for every block of the table
// without a valid hash: one thread per block, the ids formatted into the
// block's scratch (per_frag bytes per fragment: two ids, then four int32
// index entries), each orientation's list insertion-sorted, the smaller list
// folded 16 bytes at a time without being joined.
__device__ void dt_hash_one(DBlk* __restrict__ tb, const DFrag* __restrict__ tf, int64_t i, const DBlk& b,
                            const char* __restrict__ nm, const int32_t* __restrict__ nmo, int per_frag,
                            char* __restrict__ hs) {
    const int n = b.nf;
    char* buf = hs + (int64_t)b.fo * per_frag;
    int32_t* ix = (int32_t*)(buf + (int64_t)n * (per_frag - 16));  // d_off, d_len, v_off, v_len
    int32_t* doff = ix;
    int32_t* dlen = ix + n;
    int32_t* voff = ix + 2 * n;
    int32_t* vlen = ix + 3 * n;
    int p = 0;
    for (int k = 0; k < n; k++) {
        const DFrag f = tf[b.fo + k];
        const char* name = nm + nmo[f.seq];
        const int ln = nmo[f.seq + 1] - nmo[f.seq];
        for (int inv = 0; inv < 2; inv++) {
            const int ori = inv ? -f.ori : f.ori;
            const int s0 = p;
            for (int c = 0; c < ln; c++) buf[p++] = name[c];
            buf[p++] = '_';
            if (ori == 1) {
                p += fmt_i64_d(buf + p, f.min);
                buf[p++] = '_';
                p += fmt_i64_d(buf + p, f.max);
            } else {
                p += fmt_i64_d(buf + p, f.max);
                buf[p++] = '_';
                if (f.min == f.max) {
                    buf[p++] = '-';
                    buf[p++] = '1';
                } else {
                    p += fmt_i64_d(buf + p, f.min);
                }
            }
            (inv ? voff : doff)[k] = s0;
            (inv ? vlen : dlen)[k] = p - s0;
        }
    }
    for (int side = 0; side < 2; side++) {  // insertion sort of each list
        int32_t* o = side ? voff : doff;
        int32_t* l = side ? vlen : dlen;
        for (int a = 1; a < n; a++) {
            const int32_t to = o[a], tl = l[a];
            int c = a;
            for (; c > 0 && scmp_d(buf + to, tl, buf + o[c - 1], l[c - 1]) < 0; c--) {
                o[c] = o[c - 1];
                l[c] = l[c - 1];
            }
            o[c] = to;
            l[c] = tl;
        }
    }
    bool use_d = false;  // std::lexicographical_compare(d, v): d strictly less
    for (int k = 0; k < n; k++) {
        const int c = scmp_d(buf + doff[k], dlen[k], buf + voff[k], vlen[k]);
        if (c != 0) {
            use_d = c < 0;
            break;
        }
    }
    const int32_t* o = use_d ? doff : voff;
    const int32_t* l = use_d ? dlen : vlen;
    // the ids joined by ' ', padded with ' ' to 16 bytes, folded a = a*x ^ y
    uint64_t a = 1, x = 0, y = 0;
    int fill = 0;
    auto put = [&](unsigned char c) {
        if (fill < 8) x |= (uint64_t)c << (8 * fill);
        else y |= (uint64_t)c << (8 * (fill - 8));
        if (++fill == 16) {
            a = a * x;
            a ^= y;
            x = y = 0;
            fill = 0;
        }
    };
    for (int k = 0; k < n; k++) {
        if (k) put(' ');
        for (int c = 0; c < l[k]; c++) put((unsigned char)buf[o[k] + c]);
    }
    if (fill) {
        while (fill) put(' ');
    }
    tb[i].hash = a;
    tb[i].flags = b.flags | DB_HASH;
}
__global__ void k_dt_hash(DBlk* __restrict__ tb, const DFrag* __restrict__ tf, const int64_t* __restrict__ pnb,
                          const char* __restrict__ nm, const int32_t* __restrict__ nmo, int per_frag,
                          char* __restrict__ hs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *pnb) return;
    const DBlk b = tb[i];
    if (!(b.flags & DB_HASH)) dt_hash_one(tb, tf, i, b, nm, nmo, per_frag, hs);
}

// the same per block of at most 64 fragments, one wave per block: lane k
// formats fragment k's two ids into LDS, ranks them in their lists (string
// compares against every other lane's id; equal ids by lane), the first
// difference of the sorted lists picks the list, a wave prefix sum places the
// ids and their separators, and lane 0 folds the joined, padded text
static constexpr int HASH_W_NF = 64;
__device__ __forceinline__ int fmt_i64_at(char* p, int64_t x) {  // no private array (fmt_i64_d's t[24])
    const bool neg = x < 0;
    uint64_t u = neg ? (uint64_t)(-(x + 1)) + 1 : (uint64_t)x;
    int nd = 1;
    for (uint64_t t = u; t >= 10; t /= 10) nd++;
    const int w = nd + (neg ? 1 : 0);
    if (neg) p[0] = '-';
    for (int q = w - 1; q >= (neg ? 1 : 0); q--) {
        p[q] = (char)('0' + (int)(u % 10));
        u /= 10;
    }
    return w;
}
__device__ __forceinline__ int fmt_id_at(char* p, const char* name, int ln, const DFrag& f, int ori) {
    int q = 0;
    for (int c = 0; c < ln; c++) p[q++] = name[c];
    p[q++] = '_';
    if (ori == 1) {
        q += fmt_i64_at(p + q, f.min);
        p[q++] = '_';
        q += fmt_i64_at(p + q, f.max);
    } else {
        q += fmt_i64_at(p + q, f.max);
        p[q++] = '_';
        if (f.min == f.max) {
            p[q++] = '-';
            p[q++] = '1';
        } else {
            q += fmt_i64_at(p + q, f.min);
        }
    }
    return q;
}
__host__ __device__ constexpr int hash_w_lds(int idw) {  // ids [2][64][idw], joined text, orders [2][64]
    return 128 * idw + ((64 * (idw + 1) + 16 + 15) & ~15) + 128;
}
__global__ __launch_bounds__(64) void k_dt_hash_w(DBlk* __restrict__ tb, const DFrag* __restrict__ tf,
                                                  const int64_t* __restrict__ pnb, const char* __restrict__ nm,
                                                  const int32_t* __restrict__ nmo, int idw, int per_frag,
                                                  char* __restrict__ hs) {
    extern __shared__ __attribute__((aligned(16))) char lh[];
    char* ids = lh;
    char* join = lh + 128 * idw;
    uint8_t* ord = (uint8_t*)(join + ((64 * (idw + 1) + 16 + 15) & ~15));
    const int lane = threadIdx.x;
    const int64_t nb = *pnb;
    for (int64_t i = blockIdx.x; i < nb; i += gridDim.x) {
        const DBlk b = tb[i];
        if (b.flags & DB_HASH) continue;
        if (b.nf > HASH_W_NF) {  // (rare) one lane formats and sorts the ids in global scratch
            if (lane == 0) dt_hash_one(tb, tf, i, b, nm, nmo, per_frag, hs);
            continue;
        }
        const int n = b.nf;
        int len0 = 0, len1 = 0;
        if (lane < n) {
            const DFrag f = tf[b.fo + lane];
            const int s0 = nmo[f.seq], ln = nmo[f.seq + 1] - s0;
            len0 = fmt_id_at(ids + lane * idw, nm + s0, ln, f, f.ori);
            len1 = fmt_id_at(ids + (64 + lane) * idw, nm + s0, ln, f, -f.ori);
        }
        __syncthreads();
        for (int inv = 0; inv < 2; inv++) {
            const char* mine = ids + (inv * 64 + lane) * idw;
            const int ml = inv ? len1 : len0;
            int r = 0;
            for (int j = 0; j < n; j++) {
                const int lj = __shfl(inv ? len1 : len0, j);
                if (lane < n && j != lane) {
                    const int c = scmp_d(ids + (inv * 64 + j) * idw, lj, mine, ml);
                    r += c < 0 || (c == 0 && j < lane);
                }
            }
            if (lane < n) ord[inv * 64 + r] = (uint8_t)lane;
        }
        __syncthreads();
        // std::lexicographical_compare(d, v): the first position where the sorted lists differ
        const int a0 = lane < n ? ord[lane] : 0, a1 = lane < n ? ord[64 + lane] : 0;
        const int la0 = __shfl(len0, a0), la1 = __shfl(len1, a1);
        const int c = lane < n ? scmp_d(ids + a0 * idw, la0, ids + (64 + a1) * idw, la1) : 0;
        const unsigned long long ne = __ballot(c != 0);
        const int cf = ne ? __shfl(c, __ffsll((long long)ne) - 1) : 0;
        const int L = cf < 0 ? 0 : 1;  // all equal: the inverse list (either)
        const int src = L ? a1 : a0;
        const int sl = lane < n ? (L ? la1 : la0) : 0;
        const int item = lane < n ? sl + (lane > 0 ? 1 : 0) : 0;
        int off = item;  // inclusive wave prefix sum
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(off, d);
            if (lane >= d) off += t;
        }
        const int T = __shfl(off, 63);
        off -= item;
        if (lane < n) {
            char* o = join + off;
            if (lane) *o++ = ' ';
            const char* q = ids + (L * 64 + src) * idw;
            for (int k = 0; k < sl; k++) o[k] = q[k];
        }
        const int Tp = (T + 15) & ~15;
        for (int q = T + lane; q < Tp; q += 64) join[q] = ' ';
        __syncthreads();
        if (lane == 0) {
            uint64_t h = 1;
            for (int q = 0; q < Tp; q += 16) {
                const uint64_t x = *(const uint64_t*)(join + q), y = *(const uint64_t*)(join + q + 8);
                h = h * x;
                h ^= y;
            }
            tb[i].hash = h;
            tb[i].flags = b.flags | DB_HASH;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ MoveUnchanged
// MoveUnchanged::hashes_ as an open-addressing set: state 0 empty, 2 being
// written, 1 full.  Test every block, then insert the hashes of the blocks
// not held (the reference inserts this iteration's new hashes after the scan).
struct DSet {
    unsigned long long* key;
    uint32_t* st;
    uint64_t mask;
};
__device__ __forceinline__ uint64_t dset_slot(uint64_t h, uint64_t mask) {
    return ((h * 0x9E3779B97F4A7C15ull) >> 20) & mask;
}
__device__ bool dset_has(const DSet& s, uint64_t h) {
    for (uint64_t i = dset_slot(h, s.mask);; i = (i + 1) & s.mask) {
        const uint32_t st = __hip_atomic_load(&s.st[i], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if (st == 0) return false;
        if (st == 1 && s.key[i] == h) return true;
    }
}
// Pipe state: XOR of the hashes of the blocks of more than one fragment, and
// the table's row bytes and longest alignment; with it MoveUnchanged's test
// of every block against the hashes of the earlier iterations (unless the
// table is not final yet: the host runs OverlaplessUnion)
__global__ void k_dt_state(DBlk* __restrict__ tb, DSet s, ElfSum* __restrict__ sum) {
    const int64_t nb = sum->nb;
    const bool mu = !(sum->flags & (ES_OU_HOST | ES_OU_CAP));
    uint64_t h = 0;
    int64_t bytes = 0;
    int mx = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += (int64_t)gridDim.x * blockDim.x) {
        const DBlk b = tb[i];
        if (b.nf > 1) h ^= b.hash;
        if (b.flags & DB_ROWS) {
            bytes += pad16d((int64_t)b.nf * b.len);
            mx = max(mx, b.len);
        }
        if (mu) {
            const bool held = dset_has(s, b.hash);
            tb[i].flags = held ? (b.flags | DB_HELD) : (b.flags & ~DB_HELD);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        h ^= (uint64_t)__shfl_xor((unsigned long long)h, o);
        bytes += __shfl_xor((long long)bytes, o);
        mx = max(mx, __shfl_xor(mx, o));
    }
    if ((threadIdx.x & 63) == 0) {
        if (h) atomicXor((unsigned long long*)&sum->state, (unsigned long long)h);
        if (bytes) atomicAdd((unsigned long long*)&sum->bytes, (unsigned long long)bytes);
        if (mx) atomicMax(&sum->max_len, mx);
    }
}
__global__ void k_mu_insert(const DBlk* __restrict__ tb, DSet s, ElfSum* __restrict__ sum) {
    if (sum->flags & (ES_OU_HOST | ES_OU_CAP)) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sum->nb) return;
    const DBlk b = tb[i];
    if (b.flags & DB_HELD) return;
    const uint64_t h = b.hash;
    for (uint64_t k = dset_slot(h, s.mask);; k = (k + 1) & s.mask) {
        uint32_t st = __hip_atomic_load(&s.st[k], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if (st == 1 && s.key[k] == h) return;
        if (st == 0) {
            uint32_t e = 0;
            if (__hip_atomic_compare_exchange_strong(&s.st[k], &e, 2u, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
                s.key[k] = h;
                __hip_atomic_store(&s.st[k], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                atomicAdd((unsigned long long*)&sum->fresh, 1ull);
                return;
            }
        }
        // taken (a duplicate of an entry being written is harmless: membership only)
    }
}
__global__ void k_dset_rehash(DSet from, uint64_t n, DSet to) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if (from.st[i] != 1) continue;
        const uint64_t h = from.key[i];
        for (uint64_t k = dset_slot(h, to.mask);; k = (k + 1) & to.mask) {
            uint32_t e = 0;
            if (__hip_atomic_compare_exchange_strong(&to.st[k], &e, 2u, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
                to.key[k] = h;
                __hip_atomic_store(&to.st[k], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
}

// ------------------------------------------------------------------ FragmentsExtender plan
// fx_plan on the device (FragmentsExtender.cpp:34-80): for every block of at
// least two fragments with rows that MoveUnchanged did not hold, the right
// and the left flank lengths; jobs in block order (right, then left), rows
// in fragment order, flank offsets packed.
struct PlanArgs {
    const DBlk* tb;
    const DFrag* tf;
    const int64_t* seqlen;
    int32_t extend_length;
    int64_t portion;       // x 1e4
    int4* bplan;           // per block: right job, left job, right sh, left sh
    DJob* jobs;
    int2* jobsum;          // per job: rows, flank length (the host's copy)
    DRow* rows;
    int64_t* row_off;      // per row: its flank's offset and length -- the
    int32_t* row_len;      // aligner's row arrays (AlignAsync::ujobs)
    ElfSum* sum;
};
__device__ __forceinline__ void plan_block(const PlanArgs& a, const DBlk& b, int32_t (&sh)[2]) {
    sh[0] = sh[1] = 0;
    if (b.nf < 2 || !(b.flags & DB_ROWS) || (b.flags & DB_HELD)) return;
    const int64_t portion_length = a.portion * (int64_t)b.len / 10000;
    const int64_t E = max((int64_t)a.extend_length, portion_length);
    int64_t ss[2] = {E, E};
    frag_batches(a.tf + b.fo, b.nf, [&](int, const DFrag& f) {
        // max_right_shift (:34-51) of the fragment (side 0) and of its inverse (side 1)
        const int64_t r = a.seqlen[f.seq] - 1 - f.max, l = f.min;
        ss[0] = min(ss[0], f.ori == 1 ? r : l);
        ss[1] = min(ss[1], f.ori == 1 ? l : r);
    });
    for (int side = 0; side < 2; side++) {
        int64_t s = ss[side];
        if (s >= (1 << 30)) {
            atomicOr(&a.sum->flags, (int)ES_FLANK_RANGE);
            s = 0;
        }
        sh[side] = s > 0 ? (int32_t)s : 0;
    }
}
struct PlanPass {
    static constexpr int id = 0;  // (its ElfSum ticket)
    static constexpr const char* name = "plan";
    static constexpr int K = 3;  // jobs, rows, residues
    PlanArgs a;
    __device__ bool skip() const { return a.sum->flags & (ES_OU_HOST | ES_OU_CAP); }
    __device__ int64_t n() const { return a.sum->nb; }
    __device__ void count(int64_t i, int64_t (&v)[K]) const {
        int32_t sh[2];
        const DBlk b = a.tb[i];
        plan_block(a, b, sh);
        a.bplan[i] = make_int4(-1, -1, sh[0], sh[1]);  // (fill reads the flank lengths back)
        for (int s = 0; s < 2; s++)
            if (sh[s] > 0) {
                v[0]++;
                v[1] += b.nf;
                v[2] += (int64_t)b.nf * sh[s];
                if (sh[s] > __hip_atomic_load(&a.sum->max_sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                    atomicMax(&a.sum->max_sh, sh[s]);
            }
    }
    __device__ void fill(int64_t i, int64_t (&v)[K], const int64_t (&)[K]) const {
        const DBlk b = a.tb[i];
        int4 bp = a.bplan[i];  // count's flank lengths
        const int32_t sh[2] = {bp.z, bp.w};
        for (int side = 0; side < 2; side++) {
            if (sh[side] <= 0) continue;
            const int32_t j = (int32_t)v[0]++;
            (side ? bp.y : bp.x) = j;
            a.jobs[j] = DJob{(int32_t)i, side, b.nf, sh[side], v[2]};
            a.jobsum[j] = make_int2(b.nf, sh[side]);
            const int64_t r0 = v[1], b0 = v[2];
            const int32_t shs = sh[side];
            frag_batches(a.tf + b.fo, b.nf, [&](int k, const DFrag& f) {
                // f.min and f.max pinned in registers before the select: with
                // the loads sunk into the branches of the select, the ROCm 7.2
                // compiler reused the register pair of the start for the row's
                // address in the second side's copy of this loop in the
                // count / scan / fill form of the passes, since removed (each
                // row's start came out as its own address;
                // tests/test_isa_lint.py guards every kernel)
                int64_t mn = f.min, mx = f.max;
                asm volatile("" : "+v"(mn), "+v"(mx));
                const int o = side ? -f.ori : f.ori;
                const int64_t pos = o == 1 ? mx + 1 : mn - 1;
                a.rows[r0 + k] = DRow{pos, b0 + (int64_t)k * shs, f.seq, o, shs, 0};
                a.row_off[r0 + k] = b0 + (int64_t)k * shs;
                a.row_len[r0 + k] = shs;
            });
            v[1] += b.nf;
            v[2] += (int64_t)b.nf * sh[side];
        }
        a.bplan[i] = bp;
    }
    __device__ void totals(const int64_t (&tot)[K]) const {
        a.sum->nj = tot[0];
        a.sum->nrows = tot[1];
        a.sum->flank = tot[2];
    }
};

// the flank rows (k_decode with the ops made on the device): row r, piece y
__global__ void k_dt_decode(const DRow* __restrict__ rows, const int64_t* __restrict__ wofs,
                            const int64_t* __restrict__ nofs, const uint64_t* __restrict__ words,
                            const uint64_t* __restrict__ nmask, char* __restrict__ out) {
    const DRow d = rows[blockIdx.x];
    const int64_t c0 = (int64_t)blockIdx.y * PIECE;
    if (c0 >= d.len) return;
    const int64_t c1 = min((int64_t)d.len, c0 + PIECE);
    const int64_t wb = wofs[d.seq], nbse = nofs[d.seq];
    for (int64_t i = c0 + threadIdx.x; i < c1; i += blockDim.x) {
        const int64_t p = d.ori == 1 ? d.pos + i : d.pos - i;
        const uint64_t w = words[wb + (p >> 5)];
        int code = (int)((w >> (2 * (p & 31))) & 3);
        const bool isn = (nmask[nbse + (p >> 6)] >> (p & 63)) & 1;
        if (d.ori != 1) code ^= 1;
        out[d.dst + i] = isn ? 'N' : "ATGC"[code];
    }
}

// ------------------------------------------------------------------ stitch
// fx_finish on the device: every block of the table is written to the other
// arena buffer, the planned ones as revcomp(left) + row + right with their
// fragments shifted (shift_end), in table order with pad16 per block.  The
// new table (same blocks and fragments) gets the new lengths and offsets;
// a stitched block's hash is no longer valid.
struct StitchArgs {
    const DBlk* tb;
    const DFrag* tf;
    DBlk* ob;
    DFrag* of;
    int64_t nb;
    const int4* bplan;
    const DRes* res;
    ElfSum* sum;
    int4* pieces;        // (fragment, block, first column, 0) per PIECE columns of every new row
};
__device__ __forceinline__ int64_t stitch_len(const StitchArgs& a, const DBlk& b, const int4& bp) {
    int64_t L = b.len;
    if (bp.x >= 0) L += a.res[bp.x].len;
    if (bp.y >= 0) L += a.res[bp.y].len;
    return L;
}
__device__ __forceinline__ int64_t stitch_pieces(int64_t L) {  // (none past the int32 range: ES_LEN_RANGE)
    return L < (1ll << 31) ? (L + PIECE - 1) / PIECE : 0;
}
struct StitchPass {
    static constexpr int id = 1;  // (its ElfSum ticket)
    static constexpr const char* name = "stitch";
    static constexpr int K = 2;  // row bytes, copy pieces
    StitchArgs a;
    __device__ bool skip() const { return false; }
    __device__ int64_t n() const { return a.nb; }
    __device__ void count(int64_t i, int64_t (&v)[K]) const {
        const DBlk b = a.tb[i];
        if (b.flags & DB_ROWS) {
            const int64_t L = stitch_len(a, b, a.bplan[i]);
            v[0] += pad16d((int64_t)b.nf * L);
            v[1] += (int64_t)b.nf * stitch_pieces(L);
        }
    }
    __device__ void fill(int64_t i, int64_t (&v)[K], const int64_t (&)[K]) const {
        DBlk b = a.tb[i];
        const int4 bp = a.bplan[i];
        const bool ext = bp.x >= 0 || bp.y >= 0;
        const int64_t L = stitch_len(a, b, bp);
        if (L >= (1ll << 31)) atomicOr(&a.sum->flags, (int)ES_LEN_RANGE);
        const int64_t v0 = v[0];
        frag_batches<4>(a.tf + b.fo, b.nf, [&](int k, DFrag f) {
            if (bp.x >= 0) {  // right flank: shift_end in the fragment's own direction
                if (f.ori == 1) f.max += bp.z;
                else f.min -= bp.z;
            }
            if (bp.y >= 0) {  // left flank: the inverted block's right
                if (-f.ori == 1) f.max += bp.w;
                else f.min -= bp.w;
            }
            if (b.flags & DB_ROWS) f.roff = v0 + (int64_t)k * L;
            a.of[b.fo + k] = f;
        });
        if (b.flags & DB_ROWS) {
            v[0] += pad16d((int64_t)b.nf * L);
            const int64_t np = stitch_pieces(L);
            for (int k = 0; k < b.nf; k++)
                for (int64_t q = 0; q < np; q++)
                    a.pieces[v[1]++] = make_int4(b.fo + k, (int32_t)i, (int32_t)(q * PIECE), 0);
        }
        if (ext) b.flags &= ~DB_HASH;
        b.len = (int32_t)L;
        a.ob[i] = b;
    }
    __device__ void totals(const int64_t (&tot)[K]) const { a.sum->n_pieces = tot[1]; }
};

// the rows, one workgroup per piece (grid-stride over the pieces the pass listed)
__global__ __launch_bounds__(256) void k_dt_stitch_pieces(StitchArgs a, const char* __restrict__ src,
                                                          char* __restrict__ dst) {
    const int64_t np = a.sum->n_pieces;
    for (int64_t p = blockIdx.x; p < np; p += gridDim.x) {
        const int4 e = a.pieces[p];
        const int64_t r = e.x;
        const DBlk b = a.tb[e.y];
        const int k = (int)(r - b.fo);
        const int64_t L = a.ob[e.y].len;
        const int4 bp = a.bplan[e.y];
        const char* left = nullptr;
        const char* right = nullptr;
        int64_t nl = 0;
        if (bp.y >= 0) {
            const DRes q = a.res[bp.y];
            left = q.p + (int64_t)k * q.stride;
            nl = q.len;
        }
        if (bp.x >= 0) {
            const DRes q = a.res[bp.x];
            right = q.p + (int64_t)k * q.stride;
        }
        const int64_t nm = b.len;
        const char* mid = src + a.tf[r].roff;
        char* out = dst + a.of[r].roff;
        const int64_t c1 = min(L, (int64_t)e.z + PIECE);
        for (int64_t o = e.z + threadIdx.x; o < c1; o += blockDim.x) {
            char c;
            if (o < nl) c = dcompl(left[nl - 1 - o]);
            else if (o < nl + nm) c = mid[o - nl];
            else c = right[o - nl - nm];
            out[o] = c;
        }
    }
}


// ------------------------------------------------------------------ FixEnds
// column_jobs on the device: per block with rows not held, a ColJob indexed
// by the block (rows_at = its first fragment); jobs of at most
// SMALL_FE_WORDS words and SMALL_FE_ROWS rows in `list` (k_fix_ends_small),
// the others at list + nb with their tiles (k_col_bits + k_fix_ends).
struct FePlanArgs {
    const DBlk* tb;
    const DFrag* tf;
    int64_t nb;
    const char* arena;
    ColJob* jobs;
    const char** rowp;
    ColTile* tiles;
    int32_t* list;
    ElfSum* sum;
};
__device__ __forceinline__ int fe_kind(const DBlk& b) {  // 0 none, 1 small, 2 large
    if (!(b.flags & DB_ROWS) || (b.flags & DB_HELD)) return 0;
    const int64_t nw = ((int64_t)b.len + 63) >> 6;
    return (nw <= SMALL_FE_WORDS && b.nf <= SMALL_FE_ROWS) ? 1 : 2;
}
struct FePass {
    static constexpr int id = 2;  // (its ElfSum ticket)
    static constexpr const char* name = "fix_ends_plan";
    static constexpr int K = 4;  // small, large, bit words, tiles
    FePlanArgs a;
    __device__ bool skip() const { return false; }
    __device__ int64_t n() const { return a.nb; }
    __device__ void count(int64_t i, int64_t (&v)[K]) const {
        const DBlk b = a.tb[i];
        const int k = fe_kind(b);
        const int64_t nw = ((int64_t)b.len + 63) >> 6;
        if (k == 1) v[0]++;
        if (k == 2) {
            v[1]++;
            v[2] += nw;
            v[3] += (nw + TILE_WORDS - 1) / TILE_WORDS;
        }
    }
    __device__ void fill(int64_t i, int64_t (&v)[K], const int64_t (&)[K]) const {
        const DBlk b = a.tb[i];
        frag_batches(a.tf + b.fo, b.nf, [&](int k, const DFrag& f) { a.rowp[b.fo + k] = a.arena + f.roff; });
        const int k = fe_kind(b);
        if (!k) return;
        const int64_t nw = ((int64_t)b.len + 63) >> 6;
        a.jobs[i] = ColJob{(int64_t)b.fo, k == 2 ? v[2] : 0, 0, b.nf, b.len};
        if (k == 1) {
            a.list[v[0]++] = (int32_t)i;
        } else {
            a.list[a.nb + v[1]++] = (int32_t)i;
            for (int64_t w = 0; w < nw; w += TILE_WORDS)
                a.tiles[v[3]++] = ColTile{(int32_t)i, (int32_t)w, (int32_t)min(nw, w + TILE_WORDS), 0};
            v[2] += nw;
        }
    }
    __device__ void totals(const int64_t (&tot)[K]) const {
        a.sum->n_small = tot[0];
        a.sum->n_large = tot[1];
        a.sum->n_tiles = tot[3];
    }
};

// Block::slice of every block FixEnds cuts (fix_ends / slice_meta above),
// the others copied; blocks shorter than min_fragment dropped.  A 1-letter
// ori -1 slice turns ori +1 (Fragment::set_begin_last) and its row letter is
// rewritten to the forward strand's (k_set_letter, here inline).
struct SliceArgs {
    const DBlk* tb;
    const DFrag* tf;
    DBlk* ob;
    DFrag* of;
    int64_t nb;
    const int32_t* se;   // per block: start, stop-from-end
    const int32_t* cnt;  // per fragment: letters before, after
    int32_t mf;
    char* arena;
    const int64_t* wofs;
    const int64_t* nofs;
    const uint64_t* words;
    const uint64_t* nmask;
    ElfSum* sum;
};
__device__ __forceinline__ int slice_kind(const SliceArgs& a, const DBlk& b, int64_t i, int64_t& sd, int64_t& stop) {
    // 0 keep as is, 1 slice, 2 drop
    if (!(b.flags & DB_ROWS) || (b.flags & DB_HELD)) return 0;
    sd = a.se[2 * i];
    const int64_t sr = a.se[2 * i + 1];
    if (sd == 0 && sr == 0) return 0;
    stop = (int64_t)b.len - sr - 1;
    if (stop - sd + 1 < a.mf) return 2;
    return 1;
}
struct SlicePass {
    static constexpr int id = 3;  // (its ElfSum ticket)
    static constexpr const char* name = "slice";
    static constexpr int K = 2;  // blocks, fragments out
    SliceArgs a;
    __device__ bool skip() const { return false; }
    __device__ int64_t n() const { return a.nb; }
    __device__ void count(int64_t i, int64_t (&v)[K]) const {
        const DBlk b = a.tb[i];
        int64_t sd = 0, stop = 0;
        const int k = slice_kind(a, b, i, sd, stop);
        if (k == 2) return;
        v[0]++;
        if (k == 0) {
            v[1] += b.nf;
            return;
        }
#pragma unroll 8
        for (int q = 0; q < b.nf; q++) {
            const DFrag f = a.tf[b.fo + q];
            const int2 c = *(const int2*)(a.cnt + 2 * (b.fo + q));
            v[1] += (f.max - f.min + 1) - c.x - c.y > 0;
        }
    }
    __device__ void fill(int64_t i, int64_t (&v)[K], const int64_t (&)[K]) const {
        const DBlk b = a.tb[i];
        int64_t sd = 0, stop = 0;
        const int k = slice_kind(a, b, i, sd, stop);
        if (k == 2) return;
        DBlk nbk = b;
        nbk.fo = (int32_t)v[1];
        if (k == 0) {
            const int64_t o = v[1];
            frag_batches(a.tf + b.fo, b.nf,
                         [&](int q, const DFrag& f) { a.of[o + q] = DFrag{f.min, f.max, f.roff, f.seq, f.ori}; });
            v[1] += b.nf;
        } else {
            int n = 0;
            const int64_t L = stop - sd + 1;
            const int2* cnt2 = (const int2*)(a.cnt + 2 * b.fo);
            frag_batches_pre(a.tf + b.fo, b.nf, [&](int q, const DFrag&) { return cnt2[q]; },
                             [&](int q, const DFrag& f, const int2& c) {
                const int64_t before = c.x;
                const int64_t inside = (f.max - f.min + 1) - before - c.y;
                if (inside <= 0) return;
                const int64_t beg = f.ori == 1 ? f.min : f.max;
                const int64_t s0 = beg + f.ori * before, s1 = beg + f.ori * (before + inside - 1);
                DFrag g;
                g.seq = f.seq;
                g.ori = s0 <= s1 ? 1 : -1;
                g.min = min(s0, s1);
                g.max = max(s0, s1);
                g.roff = f.roff + sd;
                a.of[v[1] + n] = g;
                n++;
                if (g.ori != f.ori) {  // the row's one letter, forward strand
                    const int64_t p = g.min;
                    const uint64_t w = a.words[a.wofs[g.seq] + (p >> 5)];
                    const int code = (int)((w >> (2 * (p & 31))) & 3);
                    const bool isn = (a.nmask[a.nofs[g.seq] + (p >> 6)] >> (p & 63)) & 1;
                    const char letter = isn ? 'N' : "ATGC"[code];
                    char* row = a.arena + g.roff;
                    for (int64_t c = 0; c < L; c++)
                        if (row[c] != '-') row[c] = letter;
                }
            });
            nbk.nf = n;
            nbk.len = (int32_t)L;
            nbk.flags = n > 0 ? DB_ROWS : 0;  // a new block (no name, no hash)
            v[1] += n;
        }
        a.ob[v[0]++] = nbk;
    }
    __device__ void totals(const int64_t (&tot)[K]) const {
        a.sum->nb1 = tot[0];
        a.sum->nfr1 = tot[1];
    }
};

// ------------------------------------------------------------------ OverlaplessUnion
// OverlaplessUnion --ou-move over the table (overlapless_union above, whose
// comments have the proofs): priority = (size desc, alignment length desc,
// the smallest fragment, the sorted fragment list, rank: the blocks
// FragmentsExtender changed before the held ones) -- names are all the null
// name on this path (the host decides before the loop).  With every fragment
// inside its sequence and no block overlapping itself, SetFc never enters its
// multiset mode and a block is admitted iff no admitted block of higher
// priority shares a position with it: the lexicographically first maximal
// independent set of the conflict graph in priority order.  Conflicts come
// from one sort of every fragment by (sequence, start); each block lists the
// higher-priority blocks it conflicts with; priority sweeps then decide
// blocks whose listed blocks are decided (any admitted: rejected; all
// rejected: admitted).  Inputs outside those rules set ES_OU_HOST and the host
// runs overlapless_union instead.
struct OKey {
    int64_t size, len, fmin, fmax;
    int32_t fori, fseq;
    uint32_t tie, idx;
};
struct OLess {
    const DBlk* tb;
    const DFrag* sf;  // each block's fragments sorted by (min, max, ori, seq)
    __device__ bool operator()(const OKey& x, const OKey& y) const {
        if (x.size != y.size) return x.size > y.size;
        if (x.size < 0) return x.idx < y.idx;  // padding (no block behind it)
        if (x.len != y.len) return x.len > y.len;
        if (x.fmin != y.fmin) return x.fmin < y.fmin;
        if (x.fmax != y.fmax) return x.fmax < y.fmax;
        if (x.fori != y.fori) return x.fori < y.fori;
        if (x.fseq != y.fseq) return x.fseq < y.fseq;
        const DBlk a = tb[x.idx], b = tb[y.idx];
        for (int i = 0; i < a.nf && i < b.nf; i++) {
            const DFrag p = sf[a.fo + i], q = sf[b.fo + i];
            if (p.min != q.min) return p.min < q.min;
            if (p.max != q.max) return p.max < q.max;
            if (p.ori != q.ori) return p.ori < q.ori;
            if (p.seq != q.seq) return p.seq < q.seq;
        }
        if (a.nf != b.nf) return a.nf < b.nf;
        return x.tie < y.tie;
    }
};
// OLess's leading fields packed into 64 bits, monotone in its order: size
// descending (8 bits), alignment length descending (24 bits), the smallest
// fragment's start (32 bits).  A field past its width takes the fields
// after it to 0, so such keys tie and the full comparator orders them
// (k_ou_runs); ties are otherwise blocks whose smallest fragments start at
// the same position (of different sequences).  (With 16 / 24 / 24 bits and
// the start in 64 k units, C2's first table -- 33 k anchors of 3 fragments
// and 20 columns -- tied in runs of ~660: 80 ms of insertion sorts.)
// Padding (size -1) packs to ~0: last, in index order.
__device__ __forceinline__ uint64_t ou_prefix(const OKey& k) {
    if (k.size < 0) return ~0ull;
    const uint64_t sz = (uint64_t)min<int64_t>(k.size, 0xFF);
    uint64_t p = (0xFFull - sz) << 56;
    if (sz == 0xFF) return p;
    const uint64_t ln = (uint64_t)min<int64_t>(max<int64_t>(k.len, 0), 0xFFFFFF);
    p |= (0xFFFFFFull - ln) << 32;
    if (ln == 0xFFFFFF || k.fmin < 0) return p;
    return p | (uint64_t)min<int64_t>(k.fmin, 0xFFFFFFFF);
}
__device__ __forceinline__ bool frag_less_d(const DFrag& a, const DFrag& b) {
    if (a.min != b.min) return a.min < b.min;
    if (a.max != b.max) return a.max < b.max;
    if (a.ori != b.ori) return a.ori < b.ori;
    return a.seq < b.seq;
}
struct OuArgs {
    const DBlk* tb;
    const DFrag* tf;
    int64_t nbb, nfrb;      // bounds (the sorts run over them; keys past the counts sort last)
    const int64_t* seqlen;
    OKey* keys;
    DFrag* sf;
    int32_t* fb;            // fragment -> block
    uint64_t* fkey;         // (seq << 40) | min
    uint32_t* fval;         // fragment index
    const OKey* skeys;      // keys in priority order
    uint64_t* pkey;         // per block: the order's leading fields packed (ou_prefix), then sorted
    uint32_t* pval;         // ... the block, then the blocks in priority order (after k_ou_runs)
    uint64_t* pkey_s;
    uint32_t* pval_s;
    uint32_t* pri;          // block -> priority position
    const uint64_t* fkey_s; // fragments by (seq, min)
    const uint32_t* fval_s;
    int32_t* dcnt;          // per block: higher-priority conflicts
    int64_t* doff;
    int32_t* dcur;
    uint32_t* deps;
    int64_t deps_cap;
    uint8_t* status;        // 0 undecided, 1 admitted, 2 rejected
    int64_t* ddo;           // by priority position: the block's first listed conflict
    int32_t* ddc;           // ... and how many it has
    DBlk* ob;
    DFrag* of;
    ElfSum* sum;
};
// padding past the counts (the sorts run over the bounds): sorted last,
// never read as blocks (k_ou_fsort's grid writes it)
__device__ __forceinline__ void ou_pads(const OuArgs& a, int64_t t, int64_t stride) {
    const int64_t nb = a.sum->nb1, nfr = a.sum->nfr1;
    for (int64_t i = nb + t; i < a.nbb; i += stride) {
        OKey k{};
        k.size = -1;
        k.idx = (uint32_t)i;
        a.keys[i] = k;
        a.pkey[i] = ~0ull;
        a.pval[i] = (uint32_t)i;
    }
    for (int64_t i = nfr + t; i < a.nfrb; i += stride) {
        a.fkey[i] = ~0ull;
        a.fval[i] = (uint32_t)i;
    }
}
// keys, tie ranks (the extended blocks, then the held ones), sorted fragment
// copies, fragment sort keys, the device path's checks
struct OuPrepPass {
    static constexpr int id = 4;  // (its ElfSum ticket)
    static constexpr const char* name = "ou_prep";
    static constexpr int K = 2;  // extended (not held), held
    OuArgs a;
    __device__ bool skip() const { return false; }
    __device__ int64_t n() const { return a.sum->nb1; }
    __device__ void count(int64_t i, int64_t (&v)[K]) const { v[(a.tb[i].flags & DB_HELD) ? 1 : 0]++; }
    __device__ void fill(int64_t i, int64_t (&v)[K], const int64_t (&)[K]) const {  // (no total: k_pass_lb)
        const DBlk b = a.tb[i];
        OKey k;
        k.size = b.nf;
        k.idx = (uint32_t)i;
        // tie rank: the extended blocks in table order, then the held ones
        // (the high bit instead of an offset by the extended count: the fill
        // needs no total, so the single-launch pass can run it)
        k.tie = (b.flags & DB_HELD) ? (0x80000000u | (uint32_t)v[1]++) : (uint32_t)v[0]++;
        DFrag m{0, 0, 0, 0, 0};
        bool bad = false;
        frag_batches_pre<4>(a.tf + b.fo, b.nf, [&](int, const DFrag& f) { return a.seqlen[f.seq]; },
                         [&](int q, const DFrag& f, int64_t sl) {
            if (q == 0 || frag_less_d(f, m)) m = f;
            a.fb[b.fo + q] = (int32_t)i;
            bad |= !(f.min >= 0 && f.min <= f.max && f.max < sl) || f.seq >= (1 << 24) ||
                   f.max >= (1ll << 40);
            a.fkey[b.fo + q] = ((uint64_t)(uint32_t)f.seq << 40) | (uint64_t)(f.min & ((1ll << 40) - 1));
            a.fval[b.fo + q] = (uint32_t)(b.fo + q);
            if (b.nf > HASH_W_NF) {  // insertion into the sorted copy (smaller blocks: k_ou_fsort)
                int c = q;
                for (; c > 0 && frag_less_d(f, a.sf[b.fo + c - 1]); c--) a.sf[b.fo + c] = a.sf[b.fo + c - 1];
                a.sf[b.fo + c] = f;
            }
        });
        if (bad) atomicOr(&a.sum->flags, (int)ES_OU_HOST);
        k.len = (b.flags & DB_ROWS) ? b.len : (b.nf ? a.tf[b.fo].max - a.tf[b.fo].min + 1 : 0);
        k.fmin = m.min;
        k.fmax = m.max;
        k.fori = m.ori;
        k.fseq = m.seq;
        a.keys[i] = k;
        a.pkey[i] = ou_prefix(k);
        a.pval[i] = (uint32_t)i;
        a.dcnt[i] = 0;
        a.dcur[i] = 0;
    }
    __device__ void totals(const int64_t (&)[K]) const { a.sum->ou_in = a.sum->nb1; }
};
// each block's sorted fragment copy (and the padding), one wave per block of at most
// HASH_W_NF fragments: lane k's rank among the block's fragments (equal ones
// by lane) from shuffles, no memory traffic but the fragment in and out
__global__ __launch_bounds__(64) void k_ou_fsort(OuArgs a) {
    const int lane = threadIdx.x;
    ou_pads(a, (int64_t)blockIdx.x * 64 + lane, (int64_t)gridDim.x * 64);
    const int64_t nb = a.sum->nb1;
    for (int64_t i = blockIdx.x; i < nb; i += gridDim.x) {
        const DBlk b = a.tb[i];
        if (b.nf > HASH_W_NF || b.nf < 1) continue;
        const int n = b.nf;
        DFrag f{0, 0, 0, 0, 0};
        if (lane < n) f = a.tf[b.fo + lane];
        int r = 0;
        for (int j = 0; j < n; j++) {
            const int64_t jmin = __shfl((long long)f.min, j), jmax = __shfl((long long)f.max, j);
            const int jori = __shfl(f.ori, j), jseq = __shfl(f.seq, j);
            const DFrag g{jmin, jmax, 0, jseq, jori};
            r += frag_less_d(g, f) || (!frag_less_d(f, g) && j < lane);
        }
        if (lane < n) a.sf[b.fo + r] = f;
    }
}
// the runs of equal packed keys in the radix order, each put in OLess order
// by its first thread (insertion sort: the runs are short -- blocks of one
// size and length whose smallest fragments start at one position)
__global__ void k_ou_runs(OuArgs a, OLess less) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = a.sum->nb1;
    if (i >= n || (i > 0 && a.pkey_s[i] == a.pkey_s[i - 1])) return;
    int64_t j = i + 1;
    while (j < n && a.pkey_s[j] == a.pkey_s[i]) j++;
    for (int64_t q = i + 1; q < j; q++) {
        const uint32_t x = a.pval_s[q];
        const OKey kx = a.keys[x];
        int64_t c = q;
        for (; c > i && less(kx, a.keys[a.pval_s[c - 1]]); c--) a.pval_s[c] = a.pval_s[c - 1];
        a.pval_s[c] = x;
    }
}
// the keys in priority order, and each block's position
__global__ void k_ou_pri(OuArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.sum->nb1) return;
    const uint32_t b = a.pval_s[i];
    const_cast<OKey*>(a.skeys)[i] = a.keys[b];
    a.pri[b] = (uint32_t)i;
}
// conflicts: pass 0 counts each block's higher-priority conflicts, pass 1
// lists them; a block sharing a position with itself sends OverlaplessUnion
// to the host
__device__ __forceinline__ void ou_deps(const OuArgs& a, int64_t p, int pass) {
    const int64_t nfr = a.sum->nfr1;
    if (p >= nfr) return;
    const uint32_t r = a.fval_s[p];
    const DFrag x = a.tf[r];
    const int32_t bx = a.fb[r];
    const uint64_t sx = a.fkey_s[p] >> 40;
    for (int64_t q = p + 1; q < nfr; q++) {
        if ((a.fkey_s[q] >> 40) != sx) break;
        const uint32_t r2 = a.fval_s[q];
        const DFrag y = a.tf[r2];
        if (y.min > x.max) break;
        const int32_t by = a.fb[r2];
        if (by == bx) {
            atomicOr(&a.sum->flags, (int)ES_OU_HOST);
            return;
        }
        const bool xlow = a.pri[bx] > a.pri[by];
        const int32_t low = xlow ? bx : by, high = xlow ? by : bx;
        if (pass == 0) {
            atomicAdd(&a.dcnt[low], 1);
        } else {  // listed by priority position
            const int64_t at = a.doff[low] + atomicAdd(&a.dcur[low], 1);
            a.deps[at] = a.pri[high];
        }
    }
}
__global__ void k_ou_deps(OuArgs a) {  // pass 0 (pass 1: k_ou_deps_dd)
    if (a.sum->flags & (ES_OU_HOST | ES_OU_CAP)) return;
    ou_deps(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, 0);
}
struct OuScanPass {
    static constexpr int id = 5;  // (its ElfSum ticket)
    static constexpr const char* name = "ou_scan";
    static constexpr int K = 1;  // conflicts listed
    OuArgs a;
    __device__ bool skip() const { return a.sum->flags & (ES_OU_HOST | ES_OU_CAP); }
    __device__ int64_t n() const { return a.sum->nb1; }
    __device__ void count(int64_t i, int64_t (&v)[K]) const { v[0] += a.dcnt[i]; }
    __device__ void fill(int64_t i, int64_t (&v)[K], const int64_t (&)[K]) const {
        a.doff[i] = v[0];
        v[0] += a.dcnt[i];
    }
    __device__ void totals(const int64_t (&tot)[K]) const {
        if (tot[0] > a.deps_cap) atomicOr(&a.sum->flags, (int)ES_OU_CAP);
    }
};
// each priority position's conflict list (first, count), in priority order:
// k_ou_rounds then reads its chunks with one coalesced load each
// (launched with k_ou_deps' pass 1: k_ou_deps_dd)
__device__ __forceinline__ void ou_dd(const OuArgs& a, int64_t pos) {
    if (pos >= a.sum->nb1) return;
    const uint32_t b = a.skeys[pos].idx;
    a.ddo[pos] = a.doff[b];
    a.ddc[pos] = a.dcnt[b];
}
__global__ void k_ou_deps_dd(OuArgs a) {
    if (a.sum->flags & (ES_OU_HOST | ES_OU_CAP)) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    ou_dd(a, i);
    ou_deps(a, i, 1);
}
// greedy admission in priority order, 1024 positions at a time: within a
// chunk, rounds decide every block whose listed blocks (all of higher
// priority: earlier chunks, decided, or earlier in this chunk) are decided --
// any admitted: rejected; all rejected: admitted -- until the chunk is done
// (the highest-priority undecided block is always decidable).  Status by
// priority position, in LDS when lds_bytes holds it.
static constexpr int OU_LDS_MAX = 144 * 1024;
__global__ __launch_bounds__(WG) void k_ou_rounds(OuArgs a, int lds_bytes) {
    if (a.sum->flags & (ES_OU_HOST | ES_OU_CAP)) return;
    extern __shared__ uint8_t lst[];
    __shared__ int left;
    // a chunk is OU_PT * WG priority positions, thread t owns base + t + j * WG
    // (fewer chunks: the first iteration of a set with many blocks in long
    // conflict chains paid a few rounds of barriers per 1024 positions)
    constexpr int OU_PT = 4, OU_DREG = 4;
    constexpr int CH = OU_PT * WG;
    const int t = threadIdx.x;
    const int nb = (int)a.sum->nb1;
    volatile uint8_t* st = nb <= lds_bytes ? lst : a.status;
    for (int p = t; p < nb; p += WG) st[p] = 0;
    __syncthreads();
    // the next chunk's lists are loaded while this one is decided; a chunk
    // without conflicts (most of them) is admitted whole without rounds
    int64_t n0[OU_PT];
    int32_t nc[OU_PT];
#pragma unroll
    for (int q = 0; q < OU_PT; q++) {
        const int p = t + q * WG;
        n0[q] = p < nb ? a.ddo[p] : 0;
        nc[q] = p < nb ? a.ddc[p] : 0;
    }
    for (int base = 0; base < nb; base += CH) {
        int64_t d0[OU_PT], d1[OU_PT];
        bool mine[OU_PT];
        bool any = false;
#pragma unroll
        for (int q = 0; q < OU_PT; q++) {
            const int pos = base + t + q * WG;
            mine[q] = pos < nb;
            d0[q] = n0[q];
            d1[q] = n0[q] + nc[q];
            any |= mine[q] && d1[q] > d0[q];
            if (pos + CH < nb) {
                n0[q] = a.ddo[pos + CH];
                nc[q] = a.ddc[pos + CH];
            }
        }
        if (!__syncthreads_or(any)) {
#pragma unroll
            for (int q = 0; q < OU_PT; q++)
                if (mine[q]) st[base + t + q * WG] = 1;
            continue;
        }
        // the first OU_DREG listed blocks of each position in registers (one
        // batch of loads): the rounds then re-read only the status bytes
        uint32_t dr[OU_PT][OU_DREG];
#pragma unroll
        for (int q = 0; q < OU_PT; q++)
#pragma unroll
            for (int k = 0; k < OU_DREG; k++) dr[q][k] = (mine[q] && d0[q] + k < d1[q]) ? a.deps[d0[q] + k] : 0u;
        while (true) {
            __syncthreads();  // every thread has read the last round's `left`
            if (t == 0) left = 0;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < OU_PT; q++) {
                if (!mine[q]) continue;
                bool in = false, all_out = true;
#pragma unroll
                for (int k = 0; k < OU_DREG; k++) {
                    if (d0[q] + k >= d1[q] || in) break;
                    const uint8_t s = st[dr[q][k]];
                    if (s == 1) in = true;
                    else if (s != 2) all_out = false;
                }
                for (int64_t d = d0[q] + OU_DREG; d < d1[q] && !in; d++) {
                    const uint8_t s = st[a.deps[d]];
                    if (s == 1) {
                        in = true;
                        break;
                    }
                    if (s != 2) all_out = false;
                }
                if (in || all_out) {
                    st[base + t + q * WG] = in ? 2 : 1;
                    mine[q] = false;
                } else {
                    left = 1;
                }
            }
            __syncthreads();
            if (!left) break;
        }
    }
    if (nb <= lds_bytes)
        for (int p = t; p < nb; p += WG) a.status[p] = lst[p];
}
// the admitted blocks in priority order into the output table
struct OuCompactPass {
    static constexpr int id = 6;  // (its ElfSum ticket)
    static constexpr const char* name = "ou_compact";
    static constexpr int K = 2;  // blocks, fragments (over priority positions)
    OuArgs a;
    __device__ bool skip() const { return a.sum->flags & (ES_OU_HOST | ES_OU_CAP); }
    __device__ int64_t n() const { return a.sum->nb1; }
    __device__ void count(int64_t pos, int64_t (&v)[K]) const {
        if (a.status[pos] != 1) return;
        v[0]++;
        v[1] += a.tb[a.skeys[pos].idx].nf;
    }
    __device__ void fill(int64_t pos, int64_t (&v)[K], const int64_t (&)[K]) const {
        if (a.status[pos] != 1) return;
        DBlk k = a.tb[a.skeys[pos].idx];
        const int64_t o = v[1];
        frag_batches(a.tf + k.fo, k.nf,
                     [&](int q, const DFrag& f) { a.of[o + q] = DFrag{f.min, f.max, f.roff, f.seq, f.ori}; });
        k.fo = (int32_t)v[1];
        k.flags &= ~DB_HELD;
        a.ob[v[0]++] = k;
        v[1] += k.nf;
    }
    __device__ void totals(const int64_t (&tot)[K]) const {
        a.sum->nb = tot[0];
        a.sum->nfr = tot[1];
        a.sum->ou_rej = a.sum->nb1 - tot[0];
    }
};

// ------------------------------------------------------------------ host driver
// ------------------------------------------------------------------ anchors on the device
// DraftPangenome's first steps without a host round trip: the AnchorFinder's
// sorted FoundFragment keys (af_device_keys) -> groups (AnchorFinder.cpp:
// 356-391: a block per run of two or more equal hash indices among the kept
// keys, fragments by FoundFragment::make_fragment :240-246) -> RemoveNonStem
// --exact (RemoveNonStem.cpp:29-58: one fragment of every genome) -> the
// DummyAligner's rows (equal-length anchors: each fragment's text, reverse
// complement on the - strand) -> table 0 of the device ExtendLoopFast, in
// the order the host path builds (groups in key order, fragments in key order).
struct AncArgs {
    AfDevKeys K;
    uint64_t key_mask;
    const int32_t* genome;   // input index -> genome id (< 64)
    int32_t ng;              // genomes
    uint32_t* head;          // per key: starts a group
    uint32_t* gid;           // per key: inclusive count of group starts
    uint32_t* gstart;        // per group: first key (group G: keep)
    uint32_t* stem;          // per group (keep entries): a stem block
    uint32_t* sidx;          // ... exclusive scan: its block index
    unsigned long long* ctr; // [0] groups of >= 2 keys, [1] their keys, [2] stem blocks
    DBlk* tb;
    DFrag* tf;
    int64_t bstride;         // arena bytes per stem block: pad16(ng * k)
};
__device__ __forceinline__ void anc_frag(const AncArgs& a, uint64_t key, int32_t& seq, int64_t& mn, int32_t& ori) {
    const uint64_t key2 = key & a.key_mask;
    int lo = 0, hi = a.K.R - 1;  // the last rank whose 2 * order_off <= key2
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (2ull * a.K.meta[mid].order_off <= key2) lo = mid;
        else hi = mid - 1;
    }
    const uint64_t pos2 = key2 - 2ull * a.K.meta[lo].order_off;
    const uint64_t size = (uint64_t)a.K.meta[lo].size;
    const bool direct = pos2 < size;
    mn = (int64_t)(direct ? pos2 : pos2 - size);
    seq = a.K.by_rank[lo];
    ori = direct ? 1 : -1;
}
__global__ void k_anc_head(AncArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.K.keep) return;
    const uint64_t* k = a.K.keys;
    a.head[i] = (i == 0 || (k[i] >> a.K.key_bits) != (k[i - 1] >> a.K.key_bits)) ? 1u : 0u;
}
__global__ void k_anc_start(AncArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.K.keep) return;
    if (a.head[i]) a.gstart[a.gid[i] - 1] = (uint32_t)i;
    if (i == a.K.keep - 1) a.gstart[a.gid[i]] = (uint32_t)a.K.keep;
}
__global__ void k_anc_stem(AncArgs a) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.K.keep) return;
    const uint32_t G = a.gid[a.K.keep - 1];
    uint32_t ok = 0;
    if (g < G) {
        const uint32_t s = a.gstart[g], e = a.gstart[g + 1], n = e - s;
        if (n >= 2) {
            atomicAdd(&a.ctr[0], 1ull);
            atomicAdd(&a.ctr[1], (unsigned long long)n);
        }
        if (n >= 2 && (int32_t)n == a.ng) {  // (the AnchorFinder's blocks are groups of two or more)
            uint64_t seen = 0;
            ok = 1;
            for (uint32_t i = s; i < e && ok; i++) {
                int32_t seq, ori;
                int64_t mn;
                anc_frag(a, a.K.keys[i], seq, mn, ori);
                const uint64_t bit = 1ull << a.genome[seq];
                if (seen & bit) ok = 0;
                seen |= bit;
            }
        }
    }
    a.stem[g] = ok;
}
__global__ void k_anc_count(AncArgs a) {  // the stem blocks: the scan's total
    if (threadIdx.x == 0 && blockIdx.x == 0) a.ctr[2] = (unsigned long long)a.sidx[a.K.keep - 1] + a.stem[a.K.keep - 1];
}
__global__ void k_anc_fill(AncArgs a, int k) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.K.keep) return;
    if (!a.stem[g]) return;
    const int64_t b = a.sidx[g];
    const int32_t fo = (int32_t)(b * a.ng);
    a.tb[b] = DBlk{fo, a.ng, k, DB_ROWS, 0};
    const uint32_t s = a.gstart[g];
    for (int q = 0; q < a.ng; q++) {
        int32_t seq, ori;
        int64_t mn;
        anc_frag(a, a.K.keys[s + q], seq, mn, ori);
        a.tf[fo + q] = DFrag{mn, mn + k - 1, b * a.bstride + (int64_t)q * k, seq, ori};
    }
}
// the anchors' rows: fragment f's k letters at its roff (k_decode's rule)
__global__ void k_anc_rows(const DFrag* __restrict__ tf, int64_t nfr, int k, const int64_t* __restrict__ wofs,
                           const int64_t* __restrict__ nofs, const uint64_t* __restrict__ words,
                           const uint64_t* __restrict__ nmask, char* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nfr * k) return;
    const int64_t f = i / k;
    const int c = (int)(i - f * k);
    const DFrag d = tf[f];
    const int64_t p = d.ori == 1 ? d.min + c : d.max - c;
    const int64_t wb = wofs[d.seq], nbse = nofs[d.seq];
    const uint64_t w = words[wb + (p >> 5)];
    int code = (int)((w >> (2 * (p & 31))) & 3);
    const bool isn = (nmask[nbse + (p >> 6)] >> (p & 63)) & 1;
    if (d.ori != 1) code ^= 1;
    out[d.roff + c] = isn ? 'N' : "ATGC"[code];
}

struct ElfDev {
    DevBuf<DBlk> tb[2];
    DevBuf<DFrag> tf[2];
    DevBuf<ElfSum> sum;
    uint64_t ss_uid = 0;  // the sequence set the names / lengths below belong to
    DevBuf<char> names;
    DevBuf<int32_t> nmo;
    int per_frag = 0;
    int id_w = 0;  // k_dt_hash_w: bytes per id slot (the longest id, rounded to 8)
    DevBuf<int64_t> seqlen, wofs, nofs;
    DevBuf<char> hs;
    DevBuf<unsigned long long> setk[2];
    DevBuf<uint32_t> sets[2];
    int cs = 0;
    uint64_t set_cap = 0;
    int64_t set_n = 0;
    DevBuf<int4> bplan;
    DevBuf<DJob> jobs;
    DevBuf<int2> jobsum;
    DevBuf<DRow> rows;
    DevBuf<int64_t> row_off;  // the flank rows' offsets and lengths (the aligner's uniform jobs)
    DevBuf<int32_t> row_len;
    DevBuf<DRes> res;
    DevBuf<int4> pieces;  // the stitch's copy pieces
    DevBuf<ColJob> cj;
    DevBuf<const char*> rowp;
    DevBuf<ColTile> tiles;
    DevBuf<int32_t> list, se, cnt;
    DevBuf<uint64_t> bits;
    DevBuf<OKey> keys, skeys;
    DevBuf<uint64_t> pkey, pkey_s;
    DevBuf<uint32_t> pval, pval_s;
    DevBuf<DFrag> sf;
    DevBuf<int32_t> fb, dcnt, dcur;
    DevBuf<uint64_t> fkey, fkey_s;
    DevBuf<uint32_t> fval, fval_s, pri, deps;
    DevBuf<int64_t> doff, ddo;
    DevBuf<int32_t> ddc;
    DevBuf<uint8_t> status;
    DevBuf<char> temp;
    DevBuf<uint32_t> lbflag;        // k_pass_lb: tile flags (epoch-tagged), aggregates, inclusive prefixes
    DevBuf<char> lbagg, lbincl;
    int64_t lb_tiles = 0;
    uint32_t lb_epoch = 0;
    int64_t deps_cap = 0;
    PinnedBuf<char> h;    // the summary download
    PinnedBuf<char> hio;  // table up / downloads
    // the loop's diagnostic / test switches, read once per loop (elf_static)
    // instead of per pass: NPGX_ELF_SYNC=1 waits after every step,
    // NPGX_ELF_PASS_WG moves the single-workgroup switch (0: always the
    // multi-launch form), NPGX_ELF_PASS_MULTI=<pass> multi-launches only that pass
    bool env_sync = false;
    int64_t env_pass_wg = 2048;
    // the aligner without a host wait plans every job's re-run at the proven
    // bound ahead (3 n Σlen bytes) and the stitch arena at n Σlen a job: past
    // this many bytes an iteration takes the synchronous aligner, which sizes
    // both from the real results (NPGX_ASYNC_BUDGET_MB, default 8 GiB)
    int64_t env_async_budget = 8ll << 30;
    int env_fail_iter = -1;  // NPGX_TEST_FAIL_ELF=k: fail after iteration k's stitch (tests of the failure path)
    // the anchors' device path (anchors_to_device)
    uint64_t gen_uid = 0;
    DevBuf<int32_t> genome;
    DevBuf<uint32_t> a_head, a_gid, a_gstart, a_stem, a_sidx;
    DevBuf<unsigned long long> a_ctr;
    std::string env_pass_multi;
};

// the device loop's rules: one GPU, no blocks set aside elsewhere, blocks of
// the null name (OverlaplessUnion's name key then never decides), sizes
// within the table's int32 fields (NPGX_ELF_DEVICE=0: the host loop always,
// 1: the device loop where the rules allow; ELF_DEVICE_DEFAULT otherwise)
static constexpr bool ELF_DEVICE_DEFAULT = true;
// the set's mode and the environment allow the device loop
static bool elf_device_mode(const npgx_blockset* B) {
    const char* e = getenv("NPGX_ELF_DEVICE");  // (A/B runs: overrides the set's mode)
    if (e && e[0] == '0') return false;
    if (!(e && e[0] == '1')) {
        if (B->elf_mode == 0) return false;
        if (B->elf_mode != 1 && !ELF_DEVICE_DEFAULT) return false;
    }
    return true;
}
static bool elf_device_ok(const npgx_blockset* B) {
    if (!elf_device_mode(B)) return false;
    if (B->comm || !B->held.empty() || !B->saved.empty()) return false;
    size_t nf = 0;
    for (const Block& b : B->blocks) {
        if (b.name != NULL_BLOCK_NAME) return false;
        if (b.has_rows() && (b.len < 0 || b.len >= (1ll << 31))) return false;
        nf += b.f.size();
    }
    return nf < (1u << 31) && B->blocks.size() < (1u << 31);
}

static void elf_static(npgx_blockset* B, ElfDev& D) {
    {
        const char* e = getenv("NPGX_ELF_SYNC");
        D.env_sync = e && e[0] == '1';
        e = getenv("NPGX_ELF_PASS_WG");
        D.env_pass_wg = e ? atoll(e) : 2048;
        e = getenv("NPGX_ELF_PASS_MULTI");
        D.env_pass_multi = e ? e : "";
        e = getenv("NPGX_ASYNC_BUDGET_MB");
        D.env_async_budget = e ? atoll(e) << 20 : (8ll << 30);
        e = getenv("NPGX_TEST_FAIL_ELF");
        D.env_fail_iter = e ? atoi(e) : -1;
    }
    static const bool lds_ok =
        hipFuncSetAttribute((const void*)k_ou_rounds, hipFuncAttributeMaxDynamicSharedMemorySize, OU_LDS_MAX) ==
        hipSuccess;
    NPGX_REQUIRE(lds_ok, NPGX_ERR_HIP, "cannot enable the LDS of k_ou_rounds");
    const npgx_seqset* ss = B->ss;
    if (D.ss_uid == ss->uid) return;
    const size_t n = (size_t)ss->n;
    std::vector<int32_t> off(n + 1, 0);
    size_t maxname = 0;
    for (size_t i = 0; i < n; i++) {
        off[i + 1] = off[i] + (int32_t)ss->names[i].size();
        maxname = std::max(maxname, ss->names[i].size());
    }
    std::string cat;
    cat.reserve((size_t)off[n]);
    for (size_t i = 0; i < n; i++) cat += ss->names[i];
    std::vector<int64_t> len(n), wo(n), no(n);
    for (size_t i = 0; i < n; i++) {
        len[i] = (int64_t)ss->data[i].size();
        const int32_t r = ss->rank_of[i];
        wo[i] = ss->word_off[(size_t)r];
        no[i] = ss->n_off[(size_t)r];
    }
    D.names.ensure(std::max<size_t>(cat.size(), 1));
    D.nmo.ensure(n + 1);
    D.seqlen.ensure(n);
    D.wofs.ensure(n);
    D.nofs.ensure(n);
    if (!cat.empty()) NPGX_HIP(hipMemcpy(D.names.p, cat.data(), cat.size(), hipMemcpyHostToDevice));
    NPGX_HIP(hipMemcpy(D.nmo.p, off.data(), (n + 1) * 4, hipMemcpyHostToDevice));
    NPGX_HIP(hipMemcpy(D.seqlen.p, len.data(), n * 8, hipMemcpyHostToDevice));
    NPGX_HIP(hipMemcpy(D.wofs.p, wo.data(), n * 8, hipMemcpyHostToDevice));
    NPGX_HIP(hipMemcpy(D.nofs.p, no.data(), n * 8, hipMemcpyHostToDevice));
    D.per_frag = (int)(((2 * (maxname + 44) + 16) + 7) & ~(size_t)7);
    D.id_w = (int)((maxname + 44 + 7) & ~(size_t)7);
    D.ss_uid = ss->uid;
}

// host blocks -> table t (asynchronous; staging in D.hio, valid until the
// next sync); reserve: a run starts on them, with dt_reserve's capacities
static void dt_reserve(ElfDev& D, int64_t nb, int64_t nfr);
static void dt_upload(npgx_blockset* B, ElfDev& D, int t, const std::vector<Block>& v, int64_t& nb, int64_t& nfr,
                      bool reserve = false) {
    nb = (int64_t)v.size();
    nfr = 0;
    for (const Block& b : v) nfr += (int64_t)b.f.size();
    if (reserve) dt_reserve(D, nb, nfr);
    const size_t bb = (size_t)nb * sizeof(DBlk), fbytes = (size_t)nfr * sizeof(DFrag);
    const size_t fo = (bb + 63) & ~(size_t)63;
    char* st = D.hio.ensure(fo + fbytes + 64);
    DBlk* hb = (DBlk*)st;
    DFrag* hf = (DFrag*)(st + fo);
    int64_t k = 0;
    for (int64_t i = 0; i < nb; i++) {
        const Block& b = v[(size_t)i];
        hb[i] = DBlk{(int32_t)k, (int32_t)b.f.size(), (int32_t)(b.has_rows() ? b.len : 0),
                     (b.has_rows() ? DB_ROWS : 0) | (b.held ? DB_HELD : 0) | (b.hash_ok ? DB_HASH : 0), b.hash};
        for (size_t q = 0; q < b.f.size(); q++) {
            const Frag& f = b.f[q];
            hf[k++] = DFrag{f.min, f.max, b.has_rows() ? b.roff[q] : 0, f.seq, f.ori};
        }
    }
    D.tb[t].ensure((size_t)std::max<int64_t>(nb, 1));
    D.tf[t].ensure((size_t)std::max<int64_t>(nfr, 1));
    if (nb) NPGX_HIP(hipMemcpyAsync(D.tb[t].p, hb, bb, hipMemcpyHostToDevice, B->stream));
    if (nfr) NPGX_HIP(hipMemcpyAsync(D.tf[t].p, hf, fbytes, hipMemcpyHostToDevice, B->stream));
}

// DraftPangenome's anchors into table 0 with their DummyAligner rows (see
// "anchors on the device"); false when the AnchorFinder left no deferred
// keys or the genomes do not fit the stem test's 64-bit set (the host path
// then runs).  nb / nfr: the stem blocks and their fragments; *groups: the
// AnchorFinder's blocks (groups of two or more FoundFragments)
static ElfDev& elf_dev(npgx_blockset* B);
static bool anchors_to_device(npgx_blockset* B, npgx_af* af, int64_t& nb, int64_t& nfr, int64_t* groups) {
    AfDevKeys K;
    if (!af_device_keys(af, &K)) return false;
    ensure_genomes(B);
    if (B->n_genomes < 1 || B->n_genomes > 64 || K.keep >= (1ll << 31)) return false;
    ElfDev& D = elf_dev(B);
    hipStream_t st = B->stream;
    elf_static(B, D);
    if (D.gen_uid != B->ss->uid) {
        D.genome.ensure(B->genome.size());
        NPGX_HIP(hipMemcpy(D.genome.p, B->genome.data(), B->genome.size() * 4, hipMemcpyHostToDevice));
        D.gen_uid = B->ss->uid;
    }
    const int64_t keep = K.keep;
    const size_t n1 = (size_t)keep + 1;
    D.a_head.ensure(n1);
    D.a_gid.ensure(n1);
    D.a_gstart.ensure(n1);
    D.a_stem.ensure(n1);
    D.a_sidx.ensure(n1);
    D.a_ctr.ensure(4);
    AncArgs a;
    a.K = K;
    a.key_mask = K.key_bits >= 64 ? ~0ull : ((1ull << K.key_bits) - 1);
    a.genome = D.genome.p;
    a.ng = B->n_genomes;
    a.head = D.a_head.p;
    a.gid = D.a_gid.p;
    a.gstart = D.a_gstart.p;
    a.stem = D.a_stem.p;
    a.sidx = D.a_sidx.p;
    a.ctr = D.a_ctr.p;
    a.tb = nullptr;
    a.tf = nullptr;
    a.bstride = (int64_t)pad16((size_t)a.ng * (size_t)K.k);
    const unsigned g = (unsigned)((keep + 255) / 256);
    NPGX_HIP(hipMemsetAsync(D.a_ctr.p, 0, 32, st));
    hipLaunchKernelGGL(k_anc_head, dim3(g), dim3(256), 0, st, a);
    size_t b1 = 0, b2 = 0;
    NPGX_HIP(rocprim::inclusive_scan(nullptr, b1, D.a_head.p, D.a_gid.p, (size_t)keep, rocprim::plus<uint32_t>(), st));
    NPGX_HIP(rocprim::exclusive_scan(nullptr, b2, D.a_stem.p, D.a_sidx.p, 0u, (size_t)keep, rocprim::plus<uint32_t>(),
                                     st));
    D.temp.ensure(std::max(b1, b2) + 256);
    b1 = b2 = D.temp.cap;
    NPGX_HIP(rocprim::inclusive_scan(D.temp.p, b1, D.a_head.p, D.a_gid.p, (size_t)keep, rocprim::plus<uint32_t>(), st));
    hipLaunchKernelGGL(k_anc_start, dim3(g), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_anc_stem, dim3(g), dim3(256), 0, st, a);
    NPGX_HIP(rocprim::exclusive_scan(D.temp.p, b2, D.a_stem.p, D.a_sidx.p, 0u, (size_t)keep, rocprim::plus<uint32_t>(),
                                     st));
    // the stem count sizes the table and the rows: one download
    hipLaunchKernelGGL(k_anc_count, dim3(1), dim3(64), 0, st, a);
    NPGX_HIP(hipGetLastError());
    unsigned long long* hc = (unsigned long long*)B->pinned.take(32, st);
    NPGX_HIP(hipMemcpyAsync(hc, D.a_ctr.p, 32, hipMemcpyDeviceToHost, st));
    sync(B);
    *groups = (int64_t)hc[0];
    nb = (int64_t)hc[2];
    nfr = nb * a.ng;
    dt_reserve(D, nb, nfr);
    const int64_t total = nb * a.bstride;
    DevBuf<char>& ar = B->arena[B->cur];
    if ((size_t)total > ar.cap) ar.ensure(std::max<size_t>((size_t)total, ar.cap + ar.cap / 2));
    B->used = (size_t)total;
    a.tb = D.tb[0].p;
    a.tf = D.tf[0].p;
    hipLaunchKernelGGL(k_anc_fill, dim3(g), dim3(256), 0, st, a, K.k);
    if (nfr > 0) {
        const int64_t nc = nfr * K.k;
        hipLaunchKernelGGL(k_anc_rows, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, (const DFrag*)D.tf[0].p,
                           nfr, K.k, (const int64_t*)D.wofs.p, (const int64_t*)D.nofs.p, B->ss->words.p,
                           B->ss->nmask.p, ar.p);
    }
    NPGX_HIP(hipGetLastError());
    return true;
}

// table t -> host blocks (synchronous); held: keep the MoveUnchanged flags
static void dt_download(npgx_blockset* B, ElfDev& D, int t, int64_t nb, int64_t nfr, std::vector<Block>& v, bool held) {
    const size_t bb = (size_t)nb * sizeof(DBlk), fbytes = (size_t)nfr * sizeof(DFrag);
    const size_t fo = (bb + 63) & ~(size_t)63;
    char* st = D.hio.ensure(fo + fbytes + 64);
    if (nb) NPGX_HIP(hipMemcpyAsync(st, D.tb[t].p, bb, hipMemcpyDeviceToHost, B->stream));
    if (nfr) NPGX_HIP(hipMemcpyAsync(st + fo, D.tf[t].p, fbytes, hipMemcpyDeviceToHost, B->stream));
    sync(B);
    const DBlk* hb = (const DBlk*)st;
    const DFrag* hf = (const DFrag*)(st + fo);
    v.clear();
    v.resize((size_t)nb);
    for (int64_t i = 0; i < nb; i++) {
        const DBlk& d = hb[i];
        Block& b = v[(size_t)i];
        for (int q = 0; q < d.nf; q++) {
            const DFrag& f = hf[d.fo + q];
            b.f.push_back(Frag{f.seq, f.ori, f.min, f.max});
            if (d.flags & DB_ROWS) b.roff.push_back(f.roff);
        }
        b.len = d.len;
        b.hash = d.hash;
        b.hash_ok = (d.flags & DB_HASH) != 0;
        b.held = held && (d.flags & DB_HELD);
    }
}

static void dset_ensure(npgx_blockset* B, ElfDev& D, int64_t add) {
    const uint64_t need = 2 * (uint64_t)(D.set_n + add) + 1024;
    if (need <= D.set_cap) return;
    uint64_t cap = 1024;
    while (cap < 2 * need) cap <<= 1;
    const int o = D.cs, n = D.cs ^ 1;
    D.setk[n].ensure(cap);
    D.sets[n].ensure(cap);
    NPGX_HIP(hipMemsetAsync(D.sets[n].p, 0, cap * 4, B->stream));
    if (D.set_cap) {
        const DSet from{D.setk[o].p, D.sets[o].p, D.set_cap - 1}, to{D.setk[n].p, D.sets[n].p, cap - 1};
        hipLaunchKernelGGL(k_dset_rehash, dim3(1024), dim3(256), 0, B->stream, from, (uint64_t)D.set_cap, to);
        NPGX_HIP(hipGetLastError());
    }
    D.cs = n;
    D.set_cap = cap;
}

// a table pass over at most `bound` blocks (the count on the device may be
// smaller): one workgroup up to PASS_WG_MAX blocks, else count / scan / fill
// NPGX_ELF_SYNC=1 (diagnostic): wait for the stream after every step of the
// loop and name the step a device error surfaced in
static ElfDev& elf_dev(npgx_blockset* B);
static void esp(npgx_blockset* B, const char* what) {
    if (!elf_dev(B).env_sync) return;
    const hipError_t r = stream_wait(B->stream);
    if (r != hipSuccess)
        throw Error(NPGX_ERR_HIP, std::string("device ExtendLoopFast, after ") + what + ": " + hipGetErrorString(r));
}

static constexpr int64_t PASS_WG_MAX = 2048;
template <class P>
static void run_pass(npgx_blockset* B, ElfDev& D, const P& p, int64_t bound) {
    hipStream_t st = B->stream;
    const bool multi_only = !D.env_pass_multi.empty() && D.env_pass_multi != P::name;
    if (bound <= D.env_pass_wg || bound <= 0 || (bound <= PASS_WG_MAX && multi_only)) {
        hipLaunchKernelGGL(k_pass_wg<P>, dim3(1), dim3(WG), 0, st, p);
        NPGX_HIP(hipGetLastError());
        esp(B, P::name);
        return;
    }
    const unsigned g = (unsigned)((bound + 255) / 256);
    {
        if (D.lb_tiles < (int64_t)g) {
            D.lb_tiles = std::max<int64_t>(g, 2 * D.lb_tiles);
            D.lbflag.ensure((size_t)D.lb_tiles);
            NPGX_HIP(hipMemsetAsync(D.lbflag.p, 0, (size_t)D.lb_tiles * 4, st));
            D.lbagg.ensure((size_t)D.lb_tiles * sizeof(VK<4>));
            D.lbincl.ensure((size_t)D.lb_tiles * sizeof(VK<4>));
        }
        D.lb_epoch = (D.lb_epoch + 1) & 0x3FFFFFFFu;
        if (D.lb_epoch == 0) {  // (wrapped: old flags could match again)
            NPGX_HIP(hipMemsetAsync(D.lbflag.p, 0, (size_t)D.lb_tiles * 4, st));
            D.lb_epoch = 1;
        }
        const LbState L{D.lbflag.p, D.lbagg.p, D.lbincl.p};
        hipLaunchKernelGGL(k_pass_lb<P>, dim3(g), dim3(256), 0, st, p, L, &D.sum.p->tickets[P::id], D.lb_epoch);
        NPGX_HIP(hipGetLastError());
        esp(B, P::name);
    }
}

template <class... Bufs>
static void ensure_all(size_t n, Bufs&... bufs) {
    (bufs.ensure(n), ...);
}
// capacities for a table of nb blocks and nfr fragments (the loop never adds any)
static void dt_reserve(ElfDev& D, int64_t nb, int64_t nfr) {
    const int64_t nb0 = std::max<int64_t>(nb, 1), nfr0 = std::max<int64_t>(nfr, 1);
    D.sum.ensure(1);
    ensure_all((size_t)nb0, D.tb[0], D.tb[1], D.bplan, D.cj, D.keys, D.skeys, D.pkey, D.pkey_s, D.pval, D.pval_s,
               D.dcnt, D.dcur, D.doff, D.ddo, D.ddc, D.pri, D.status);
    ensure_all((size_t)(2 * nb0), D.jobs, D.jobsum, D.res, D.list, D.se);
    ensure_all((size_t)nfr0, D.tf[0], D.tf[1], D.rowp, D.sf, D.fb, D.fkey, D.fkey_s, D.fval, D.fval_s);
    ensure_all((size_t)(2 * nfr0), D.rows, D.row_off, D.row_len, D.cnt);
    D.hs.ensure((size_t)nfr0 * (size_t)D.per_frag);
    if (D.deps_cap < 8 * nfr0 + (1 << 20)) {
        D.deps_cap = 8 * nfr0 + (1 << 20);
        D.deps.ensure((size_t)D.deps_cap);
    }
}

// hash, Pipe state, MoveUnchanged, the next plan on table t (counts in the
// device summary), then the one download: the summary and the planned jobs
static const ElfSum& elf_tail(npgx_blockset* B, ElfDev& D, int t, int64_t nb_bound, const int2*& jobsum,
                              double& wait_ms) {
    hipStream_t st = B->stream;
    const unsigned nbg = (unsigned)std::max<int64_t>(1, (nb_bound + 63) / 64);
    // blocks of at most HASH_W_NF fragments one wave each, larger ones one thread each
    const bool wave_hash = hash_w_lds(D.id_w) <= 64 * 1024;
    if (wave_hash)
        hipLaunchKernelGGL(k_dt_hash_w, dim3((unsigned)std::min<int64_t>(std::max<int64_t>(nb_bound, 1), 8192)),
                           dim3(64), (size_t)hash_w_lds(D.id_w), st, D.tb[t].p, D.tf[t].p, &D.sum.p->nb, D.names.p,
                           D.nmo.p, D.id_w, D.per_frag, D.hs.p);
    else
        hipLaunchKernelGGL(k_dt_hash, dim3(nbg), dim3(64), 0, st, D.tb[t].p, D.tf[t].p, &D.sum.p->nb, D.names.p,
                           D.nmo.p, D.per_frag, D.hs.p);
    esp(B, "block_hash");
    dset_ensure(B, D, nb_bound);
    const DSet s{D.setk[D.cs].p, D.sets[D.cs].p, D.set_cap - 1};
    hipLaunchKernelGGL(k_dt_state, dim3((unsigned)std::min<int64_t>(256, (nb_bound + 255) / 256 + 1)), dim3(256), 0, st,
                       D.tb[t].p, s, D.sum.p);
    hipLaunchKernelGGL(k_mu_insert, dim3(nbg), dim3(64), 0, st, D.tb[t].p, s, D.sum.p);
    esp(B, "move_unchanged");
    PlanArgs pa{D.tb[t].p, D.tf[t].p, D.seqlen.p, B->opt.extend_length, 5000,
                D.bplan.p, D.jobs.p, D.jobsum.p, D.rows.p, D.row_off.p, D.row_len.p, D.sum.p};
    run_pass(B, D, PlanPass{pa}, nb_bound);
    NPGX_HIP(hipGetLastError());
    const size_t jb = (size_t)2 * (size_t)std::max<int64_t>(nb_bound, 1) * sizeof(int2);
    char* h = D.h.ensure(sizeof(ElfSum) + 64 + jb);
    NPGX_HIP(hipMemcpyAsync(h, D.sum.p, sizeof(ElfSum), hipMemcpyDeviceToHost, st));
    NPGX_HIP(hipMemcpyAsync(h + sizeof(ElfSum) + 64, D.jobsum.p, jb, hipMemcpyDeviceToHost, st));
    auto tw = Clock::now();
    NPGX_HIP(stream_wait(st));
    wait_ms += ms_since(tw);
    jobsum = (const int2*)(h + sizeof(ElfSum) + 64);
    return *(const ElfSum*)h;
}

// NPGX_ELF_CHECK=1 (diagnostic): after every summary download, table t and
// the planned flank rows are checked on the host -- compact fragment runs,
// fragments inside their sequences, rows inside the arena, flank rows inside
// their sequences and the flank buffer -- so that a wrong offset fails loudly
// instead of faulting the kernels that read it
static void dt_check(npgx_blockset* B, ElfDev& D, int t, const ElfSum& S, int it) {
    const char* e = getenv("NPGX_ELF_CHECK");
    const bool on = e && e[0] == '1';
    if (!on || (S.flags & (ES_OU_HOST | ES_OU_CAP))) return;
    NPGX_HIP(stream_wait(B->stream));
    std::vector<DBlk> hb((size_t)S.nb);
    std::vector<DFrag> hf((size_t)S.nfr);
    std::vector<DRow> hr((size_t)S.nrows);
    NPGX_REQUIRE(S.nb >= 0 && (size_t)S.nb <= D.tb[t].cap && S.nfr >= 0 && (size_t)S.nfr <= D.tf[t].cap &&
                     S.nrows >= 0 && (size_t)S.nrows <= D.rows.cap,
                 NPGX_ERR_STATE, "elf check: counts past the capacities");
    if (S.nb) NPGX_HIP(hipMemcpy(hb.data(), D.tb[t].p, hb.size() * sizeof(DBlk), hipMemcpyDeviceToHost));
    if (S.nfr) NPGX_HIP(hipMemcpy(hf.data(), D.tf[t].p, hf.size() * sizeof(DFrag), hipMemcpyDeviceToHost));
    if (S.nrows) NPGX_HIP(hipMemcpy(hr.data(), D.rows.p, hr.size() * sizeof(DRow), hipMemcpyDeviceToHost));
    const npgx_seqset* ss = B->ss;
    const int64_t arena = (int64_t)B->arena[B->cur].cap;
    char msg[512];
    int64_t fo = 0;
    for (int64_t i = 0; i < S.nb; i++) {
        const DBlk& b = hb[(size_t)i];
        if (b.fo != fo || b.nf < 0 || fo + b.nf > S.nfr) {
            snprintf(msg, sizeof msg, "elf check: block %lld fo %d nf %d (expected fo %lld, nfr %lld)", (long long)i,
                     b.fo, b.nf, (long long)fo, (long long)S.nfr);
            NPGX_REQUIRE(false, NPGX_ERR_STATE, msg);
        }
        for (int k = 0; k < b.nf; k++) {
            const DFrag& f = hf[(size_t)(fo + k)];
            const bool ok = f.seq >= 0 && f.seq < ss->n && (f.ori == 1 || f.ori == -1) && 0 <= f.min &&
                            f.min <= f.max && f.max < (int64_t)ss->data[(size_t)f.seq].size() &&
                            (!(b.flags & DB_ROWS) || (f.roff >= 0 && f.roff + b.len <= arena));
            if (!ok) {
                snprintf(msg, sizeof msg, "elf check: block %lld frag %d seq %d ori %d [%lld, %lld] roff %lld len %d",
                         (long long)i, k, f.seq, f.ori, (long long)f.min, (long long)f.max, (long long)f.roff, b.len);
                NPGX_REQUIRE(false, NPGX_ERR_STATE, msg);
            }
        }
        fo += b.nf;
    }
    NPGX_REQUIRE(fo == S.nfr, NPGX_ERR_STATE, "elf check: fragment count");
    for (int64_t r = 0; r < S.nrows; r++) {
        const DRow& d = hr[(size_t)r];
        const bool sq = d.seq >= 0 && d.seq < ss->n;
        const int64_t L = sq ? (int64_t)ss->data[(size_t)d.seq].size() : 0;
        const int64_t lo = d.ori == 1 ? d.pos : d.pos - d.len + 1, hi = d.ori == 1 ? d.pos + d.len - 1 : d.pos;
        const bool ok = sq && (d.ori == 1 || d.ori == -1) && d.len > 0 && d.len <= S.max_sh && lo >= 0 && hi < L &&
                        d.dst >= 0 && d.dst + d.len <= S.flank;
        if (!ok) {
            // the job and the block that planned the row
            std::vector<DJob> hj((size_t)S.nj);
            if (S.nj) NPGX_HIP(hipMemcpy(hj.data(), D.jobs.p, hj.size() * sizeof(DJob), hipMemcpyDeviceToHost));
            int64_t base = 0, j = 0;
            while (j < S.nj && base + hj[(size_t)j].nf <= r) base += hj[(size_t)j++].nf;
            std::string blk = "?";
            if (j < S.nj && hj[(size_t)j].block >= 0 && hj[(size_t)j].block < S.nb) {
                const DBlk& b = hb[(size_t)hj[(size_t)j].block];
                const int k = (int)(r - base);
                const DFrag& f = hf[(size_t)(b.fo + std::min(k, std::max(b.nf - 1, 0)))];
                blk = "block " + std::to_string(hj[(size_t)j].block) + " side " + std::to_string(hj[(size_t)j].side) +
                      " nf " + std::to_string(b.nf) + " fo " + std::to_string(b.fo) + " frag " + std::to_string(k) +
                      " [" + std::to_string(f.min) + "," + std::to_string(f.max) + "] ori " + std::to_string(f.ori) +
                      " seq " + std::to_string(f.seq);
            }
            snprintf(msg, sizeof msg, "elf check (iteration %d): flank row %lld seq %d ori %d pos %lld len %d dst %lld "
                     "(flank %lld, max_sh %d, nj %lld, nrows %lld) job %lld: %s", it, (long long)r, d.seq, d.ori,
                     (long long)d.pos, d.len, (long long)d.dst, (long long)S.flank, S.max_sh, (long long)S.nj,
                     (long long)S.nrows, (long long)j, blk.c_str());
            NPGX_REQUIRE(false, NPGX_ERR_STATE, msg);
        }
    }
}

// a zeroed summary with these counts to D.sum: nb / nfr, the table the tail
// reads, or (ou_input) nb1 / nfr1, the table OverlaplessUnion reads
static void sum_upload(npgx_blockset* B, ElfDev& D, int64_t nb, int64_t nfr, bool ou_input = false) {
    ElfSum* hs = (ElfSum*)B->pinned.take(sizeof(ElfSum), B->stream);
    *hs = ElfSum{};
    (ou_input ? hs->nb1 : hs->nb) = nb;
    (ou_input ? hs->nfr1 : hs->nfr) = nfr;
    NPGX_HIP(hipMemcpyAsync(D.sum.p, hs, sizeof(ElfSum), hipMemcpyHostToDevice, B->stream));
}

// ES_OU_CAP: more conflicts than the dependency list holds (the host ran
// this OverlaplessUnion); the next one gets a list four times as long
static void deps_grow_if_full(ElfDev& D, const ElfSum& S) {
    if (!(S.flags & ES_OU_CAP)) return;
    D.deps_cap *= 4;
    D.deps.ensure((size_t)D.deps_cap);
}

// OverlaplessUnion's arguments: table t (at most nb blocks / nfr fragments) into table t ^ 1
static OuArgs ou_args(ElfDev& D, int t, int64_t nb, int64_t nfr) {
    OuArgs oa;
    oa.tb = D.tb[t].p;
    oa.tf = D.tf[t].p;
    oa.nbb = nb;
    oa.nfrb = nfr;
    oa.seqlen = D.seqlen.p;
    oa.keys = D.keys.p;
    oa.sf = D.sf.p;
    oa.fb = D.fb.p;
    oa.fkey = D.fkey.p;
    oa.fval = D.fval.p;
    oa.skeys = D.skeys.p;
    oa.pkey = D.pkey.p;
    oa.pval = D.pval.p;
    oa.pkey_s = D.pkey_s.p;
    oa.pval_s = D.pval_s.p;
    oa.pri = D.pri.p;
    oa.fkey_s = D.fkey_s.p;
    oa.fval_s = D.fval_s.p;
    oa.dcnt = D.dcnt.p;
    oa.doff = D.doff.p;
    oa.dcur = D.dcur.p;
    oa.deps = D.deps.p;
    oa.deps_cap = D.deps_cap;
    oa.status = D.status.p;
    oa.ddo = D.ddo.p;
    oa.ddc = D.ddc.p;
    oa.ob = D.tb[t ^ 1].p;
    oa.of = D.tf[t ^ 1].p;
    oa.sum = D.sum.p;
    return oa;
}

// OverlaplessUnion of table t (counts nb1 / nfr1 in the summary, at most
// nb / nfr) into table t ^ 1 (counts nb / nfr in the summary); ES_OU_HOST or
// ES_OU_CAP in the summary: not done, the host must run it
static void dt_ou_launch(npgx_blockset* B, ElfDev& D, int t, int64_t nb, int64_t nfr) {
    hipStream_t st = B->stream;
    const OuArgs oa = ou_args(D, t, nb, nfr);
    run_pass(B, D, OuPrepPass{oa}, nb);
    NPGX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ou_fsort, dim3((unsigned)std::min<int64_t>(std::max<int64_t>(nb, 1), 8192)), dim3(64), 0, st,
                       oa);
    esp(B, "ou_prep");
    if (nb > 1 || nfr > 1) {  // (one block of many fragments: its fragments sorted all the same)
        size_t b1 = 0, b2 = 0;
        if (nb > 1)
            NPGX_HIP(rocprim::radix_sort_pairs(nullptr, b1, D.pkey.p, D.pkey_s.p, D.pval.p, D.pval_s.p, (size_t)nb, 0,
                                               64, st));
        if (nfr > 1)
            NPGX_HIP(rocprim::radix_sort_pairs(nullptr, b2, D.fkey.p, D.fkey_s.p, D.fval.p, D.fval_s.p,
                                               (size_t)nfr, 0, 64, st));
        D.temp.ensure(std::max(b1, b2) + 256);
        b1 = b2 = D.temp.cap;
        if (nb > 1)
            NPGX_HIP(rocprim::radix_sort_pairs(D.temp.p, b1, D.pkey.p, D.pkey_s.p, D.pval.p, D.pval_s.p, (size_t)nb, 0,
                                               64, st));
        if (nfr > 1)
            NPGX_HIP(rocprim::radix_sort_pairs(D.temp.p, b2, D.fkey.p, D.fkey_s.p, D.fval.p, D.fval_s.p,
                                               (size_t)nfr, 0, 64, st));
    }
    esp(B, "ou_sorts");
    if (nb <= 1) {
        NPGX_HIP(hipMemcpyAsync(D.pkey_s.p, D.pkey.p, 8, hipMemcpyDeviceToDevice, st));
        NPGX_HIP(hipMemcpyAsync(D.pval_s.p, D.pval.p, 4, hipMemcpyDeviceToDevice, st));
    }
    if (nfr <= 1) {
        NPGX_HIP(hipMemcpyAsync(D.fkey_s.p, D.fkey.p, 8, hipMemcpyDeviceToDevice, st));
        NPGX_HIP(hipMemcpyAsync(D.fval_s.p, D.fval.p, 4, hipMemcpyDeviceToDevice, st));
    }
    const unsigned nbt = (unsigned)std::max<int64_t>(1, (nb + 255) / 256), nft = (unsigned)std::max<int64_t>(1, (nfr + 255) / 256);
    hipLaunchKernelGGL(k_ou_runs, dim3(nbt), dim3(256), 0, st, oa, OLess{D.tb[t].p, D.sf.p});
    hipLaunchKernelGGL(k_ou_pri, dim3(nbt), dim3(256), 0, st, oa);
    hipLaunchKernelGGL(k_ou_deps, dim3(nft), dim3(256), 0, st, oa);
    esp(B, "ou_deps");
    run_pass(B, D, OuScanPass{oa}, nb);
    hipLaunchKernelGGL(k_ou_deps_dd, dim3(std::max(nbt, nft)), dim3(256), 0, st, oa);
    const int lds = (int)std::min<int64_t>(nb, OU_LDS_MAX);
    hipLaunchKernelGGL(k_ou_rounds, dim3(1), dim3(WG), (size_t)lds, st, oa, lds);
    esp(B, "ou_rounds");
    run_pass(B, D, OuCompactPass{oa}, nb);
    NPGX_HIP(hipGetLastError());
}

static ElfDev& elf_dev(npgx_blockset* B) {
    npgx_blockset* owner = B->elf_lender ? B->elf_lender : B;
    if (!owner->elf) owner->elf = new ElfDev;
    return *owner->elf;
}

// The loop's entry state, kept for a failure: B->blocks stays the entry copy
// until the final download, and its rows stay in arena[cur]: the first
// stitch writes the other buffer, and before the second (which would write
// arena[cur]) the entry buffer is swapped out into arena_x.
struct ElfEntry {
    int cur;
    size_t used;
    bool swapped;
};

// One run of the device loop (the counterpart of SaCall in
// similar_aligner.hip): the state its steps share, and the steps in the order
// extend_loop_fast_dev_run calls them.  Every step of an iteration books its
// host time to its ms_stage and ends on its mark of the stage clock.
struct ElfLoop {
    npgx_blockset* const B;
    ElfDev& D;
    const hipStream_t st;
    ElfEntry& E;
    int t = 0;                        // the current table: a step reads it, writes the other one and flips
    ElfSum S{};                       // the last summary downloaded ...
    const int2* js = nullptr;         // ... and its planned jobs (rows, row length), valid until the next download
    double wait_ms = 0;               // the host's waits for the stream so far
    std::set<uint64_t> states;        // the Pipe's states seen
    bool times_pending = false;       // aligner timers not read yet (async iterations)
    const bool per_iteration_stats;   // (per-job statistics: each launch's)
    // the iteration's values
    int it = -1;
    int64_t nb = 0, nfr = 0, nj = 0;  // the table's blocks and fragments, the planned jobs
    int64_t bound = 0, maxres = 0;    // bounds: the stitched rows' bytes, the longest flank alignment
    bool async = false;               // the aligner runs without a host wait
    Clock::time_point t_iter;
    double wait0 = 0, align_ms = 0;
    // the synchronous aligner's host arrays (their capacity outlives the iteration)
    std::vector<int64_t> row_off;
    std::vector<int32_t> row_len, job_start;

    ElfLoop(npgx_blockset* B_, ElfEntry& E_)
        : B(B_), D(elf_dev(B_)), st(B_->stream), E(E_), per_iteration_stats(aligner_wants_stats(B_->aligner)) {}

    void flip() { t ^= 1; }

    // hash, Pipe state, MoveUnchanged and the next plan on the current table
    // (elf_tail), with the loop's one host wait
    void plan(int64_t nb_bound) {
        S = elf_tail(B, D, t, nb_bound, js, wait_ms);
        B->pinned.reset();
        dt_check(B, D, t, S, it);
    }

    // The loop's switches and the set's names, the blocks into table 0 (pre_nb
    // >= 0: anchors_to_device left them there), an empty MoveUnchanged set,
    // the first summary and the first plan
    void enter(int64_t pre_nb, int64_t pre_nfr) {
        auto t0 = Clock::now();
        elf_static(B, D);
        nb = pre_nb, nfr = pre_nfr;
        if (pre_nb < 0) dt_upload(B, D, 0, B->blocks, nb, nfr, true);
        D.set_cap = 0;
        D.set_n = 0;
        sum_upload(B, D, nb, nfr);
        B->clock.mark(st, GS_ELF_UPLOAD);
        plan(nb);
        D.set_n += S.fresh;
        states.insert(S.state);
        B->stats.ms_host += ms_since(t0);
    }

    // An iteration starts: the last plan gives its counts, the device summary
    // starts from zero, and the planned flank rows are decoded into B->flank
    void decode_flanks(int iteration) {
        it = iteration;
        B->stats.iterations++;
        B->stats.device_iterations++;
        t_iter = Clock::now();
        wait0 = wait_ms;
        NPGX_REQUIRE(!(S.flags & ES_FLANK_RANGE), NPGX_ERR_RANGE, "flank too long");
        nj = S.nj;
        nb = S.nb;
        nfr = S.nfr;
        B->stats.aligned_residues += S.flank;
        B->stats.align_jobs += nj;
        NPGX_HIP(hipMemsetAsync(D.sum.p, 0, sizeof(ElfSum), st));
        B->flank.grow2((size_t)std::max<int64_t>(S.flank, 1));
        B->clock.mark(st, GS_ELF_PLAN);
        if (S.nrows) {
            hipLaunchKernelGGL(k_dt_decode, dim3((unsigned)S.nrows, (unsigned)((S.max_sh + PIECE - 1) / PIECE)),
                               dim3(256), 0, st, D.rows.p, D.wofs.p, D.nofs.p, B->ss->words.p, B->ss->nmask.p,
                               B->flank.p);
            NPGX_HIP(hipGetLastError());
            esp(B, "flank decode");
        }
        B->clock.mark(st, GS_FLANK_DECODE);
        B->stats.ms_stage[ST_FLANK_GATHER] += ms_since(t_iter);
    }

    // The flank jobs through the aligner, asynchronous where every job has at
    // most 64 rows and the batch fits the budget; either way the results are
    // in D.res, and bound / maxres cover them
    void align() {
        auto ta = Clock::now();
        AlignResult& res = B->fx.res;
        bound = S.bytes + 16 * nb + 64;
        maxres = 0;
        bool wide = false;
        int64_t async_bytes = 0;
        for (int64_t j = 0; j < nj; j++) {
            wide |= js[j].x > 64;
            const int64_t n = js[j].x, rs = (int64_t)js[j].x * js[j].y;
            async_bytes += ((3 * n * rs + 255) & ~255ll) + n * rs;
        }
        async = nj && !wide && async_bytes <= D.env_async_budget;
        if (async) {
            // no host wait: the aligner re-runs overflowed jobs and writes every
            // job's rows to D.res on the device; the bounds use the proven
            // column bound (the rows' total length).  Its row arrays are the
            // plan's (PlanPass): the host passes each job's rows and length only.
            // Its kernel timers accumulate over the iterations and are read
            // once after the loop (reading them is a host round of event
            // queries between the iteration's download and the next launch)
            if (!times_pending) aligner_timer_reset(B->aligner);
            times_pending = true;
            AlignAsync as{D.res.p, &D.sum.p->align_err, &D.sum.p->align_epoch};
            as.ujobs = js;
            as.d_row_off = D.row_off.p;
            as.d_row_len = D.row_len.p;
            align_device(B->aligner, B->flank.p, nullptr, nullptr, nullptr, (int32_t)nj, res, &as);
            for (int64_t j = 0; j < nj; j++) {
                const int64_t sum = (int64_t)js[j].x * js[j].y;
                bound += (int64_t)js[j].x * sum;
                maxres = std::max(maxres, sum);
            }
            double prep = 0, wait = 0;
            aligner_host_ms(B->aligner, &prep, &wait);
            B->stats.ms_stage[ST_ALIGN_HOST_PREP] += prep;
        } else if (nj) {
            B->stats.device_sync_iterations++;
            sync_rows();
            if (times_pending) collect_aligner(B);
            times_pending = false;
            aligner_timer_reset(B->aligner);
            align_device(B->aligner, B->flank.p, row_off.data(), row_len.data(), job_start.data(), (int32_t)nj, res);
            collect_aligner(B);
            double prep = 0, wait = 0;
            aligner_host_ms(B->aligner, &prep, &wait);
            B->stats.ms_stage[ST_ALIGN_HOST_PREP] += prep;
            B->stats.ms_stage[ST_DEVICE_WAIT] += wait;
            DRes* hr = (DRes*)B->pinned.take((size_t)nj * sizeof(DRes), st);
            for (int64_t j = 0; j < nj; j++) {
                hr[j] = DRes{res.bptr[(size_t)j], res.cap[(size_t)j], res.len[(size_t)j]};
                bound += (int64_t)js[j].x * res.len[(size_t)j];
                maxres = std::max<int64_t>(maxres, res.len[(size_t)j]);
            }
            NPGX_HIP(hipMemcpyAsync(D.res.p, hr, (size_t)nj * sizeof(DRes), hipMemcpyHostToDevice, st));
        }
        esp(B, "align");
        B->clock.mark(st, GS_ALIGN);
        align_ms = ms_since(ta);
        B->stats.ms_align += align_ms;
        B->stats.ms_stage[ST_ALIGN_BATCH] += align_ms;
    }

    // the batch's host arrays for the synchronous align_device (row r of job j at base + i * sh)
    void sync_rows() {
        row_off.resize((size_t)S.nrows);
        row_len.resize((size_t)S.nrows);
        job_start.assign(1, 0);
        int64_t base = 0, r = 0;
        for (int64_t j = 0; j < nj; j++) {
            const int2 q = js[j];
            for (int i = 0; i < q.x; i++) {
                row_off[(size_t)r] = base;
                row_len[(size_t)r] = q.y;
                base += q.y;
                r++;
            }
            job_start.push_back((int32_t)r);
        }
    }

    // Every block's rows with its flank alignments on both sides, into the
    // other arena buffer and the other table.  Never into the entry rows'
    // buffer: before the second stitch would, that buffer is swapped out
    // into arena_x (ElfEntry)
    void stitch() {
        auto tr = Clock::now();
        if ((B->cur ^ 1) == E.cur && !E.swapped) {
            B->arena[E.cur].swap(B->arena_x);
            E.swapped = true;
        }
        DevBuf<char>& o = B->arena[B->cur ^ 1];
        o.grow2((size_t)bound, (size_t)bound + (size_t)bound / 4 + 4096);
        // pieces: sum over the rows of ceil(length / PIECE) <= bytes / PIECE + rows
        const int64_t piece_cap = bound / PIECE + nfr + 1;
        D.pieces.grow2((size_t)piece_cap);
        const StitchArgs sa{D.tb[t].p, D.tf[t].p, D.tb[t ^ 1].p, D.tf[t ^ 1].p, nb, D.bplan.p, D.res.p, D.sum.p,
                            D.pieces.p};
        run_pass(B, D, StitchPass{sa}, nb);
        if (nfr) {
            size_t tk = B->timer.begin("stitch_rows", st, 2.0 * (double)bound, bound);
            hipLaunchKernelGGL(k_dt_stitch_pieces, dim3((unsigned)std::min<int64_t>(piece_cap, 16384)), dim3(256), 0,
                               st, sa, B->base(), o.p);
            B->timer.end(tk, st);
        }
        NPGX_HIP(hipGetLastError());
        esp(B, "stitch copy");
        B->clock.mark(st, GS_STITCH);
        B->cur ^= 1;
        B->used = (size_t)bound;
        flip();
        NPGX_REQUIRE(it != D.env_fail_iter, NPGX_ERR_STATE, "injected ExtendLoopFast failure (NPGX_TEST_FAIL_ELF)");
        B->stats.ms_stage[ST_STITCH] += ms_since(tr);
    }

    // FixEnds on the stitched blocks (the job lists and tiles planned on the
    // device), then the slicing into the other table
    void fix_ends() {
        auto tf = Clock::now();
        const int64_t bits_bound = bound / 64 + nb + 1;
        D.bits.grow2((size_t)bits_bound);
        D.tiles.ensure((size_t)(bits_bound / TILE_WORDS + nb + 1));
        const FePlanArgs fa{D.tb[t].p, D.tf[t].p, nb, B->base(), D.cj.p, D.rowp.p, D.tiles.p, D.list.p, D.sum.p};
        run_pass(B, D, FePass{fa}, nb);
        FeArgs A = fe_args(B);
        A.jobs = D.cj.p;
        A.rowp = D.rowp.p;
        A.bits = D.bits.p;
        A.out_se = D.se.p;
        A.out_cnt = D.cnt.p;
        const int64_t maxL = (int64_t)S.max_len + 2 * maxres + 1;
        A.lds_words = (int)std::min<int64_t>((maxL + 63) / 64, 4096);
        const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>(nb, 2048));
        size_t tk = B->timer.begin("fix_ends", st, 0.0, 0);
        hipLaunchKernelGGL(k_fix_ends_small, dim3(g), dim3(256), 0, st, A, D.list.p, 0, &D.sum.p->n_small);
        hipLaunchKernelGGL(k_col_bits, dim3(2048), dim3(256), 0, st, D.tiles.p, D.cj.p, D.rowp.p, D.bits.p, 0,
                           &D.sum.p->n_tiles);
        hipLaunchKernelGGL(k_fix_ends, dim3(g), dim3(256), (size_t)A.lds_words * 8, st, A, D.list.p + nb,
                           &D.sum.p->n_large);
        B->timer.end(tk, st);
        NPGX_HIP(hipGetLastError());
        esp(B, "fix_ends");
        const SliceArgs sl{D.tb[t].p, D.tf[t].p, D.tb[t ^ 1].p, D.tf[t ^ 1].p, nb, D.se.p, D.cnt.p, A.mf, B->base(),
                           D.wofs.p, D.nofs.p, B->ss->words.p, B->ss->nmask.p, D.sum.p};
        run_pass(B, D, SlicePass{sl}, nb);
        NPGX_HIP(hipGetLastError());
        B->clock.mark(st, GS_FIX_ENDS);
        flip();
        B->stats.ms_stage[ST_FIX_ENDS] += ms_since(tf);
    }

    // OverlaplessUnion --ou-move of the sliced table into the other one
    void overlapless_union() {
        auto to = Clock::now();
        dt_ou_launch(B, D, t, nb, nfr);
        B->clock.mark(st, GS_OVERLAPLESS_UNION);
        flip();
        B->stats.ms_stage[ST_OVERLAPLESS_UNION] += ms_since(to);
    }

    // The iteration's one download: the next plan with the iteration's
    // verdicts (OverlaplessUnion left to the host, the aligner's and the
    // lengths' range errors).  True: the Pipe's state was seen before, the
    // loop is done
    bool tail() {
        auto th = Clock::now();
        plan(nb);
        const int32_t align_err = S.align_err, len_err = S.flags & ES_LEN_RANGE;
        if (async) aligner_note_epoch(B->aligner, S.align_epoch);
        if (S.flags & (ES_OU_HOST | ES_OU_CAP)) {
            ou_on_host();
        } else {
            B->stats.counters[CT_OU_IN] += S.ou_in;
            B->stats.counters[CT_OU_REJECTED] += S.ou_rej;
        }
        NPGX_REQUIRE(!len_err, NPGX_ERR_RANGE, "alignment too long");
        NPGX_REQUIRE(align_err == 0, NPGX_ERR_RANGE, "alignment exceeded the proven column bound");
        if (async && per_iteration_stats) {  // (its events are complete now)
            collect_aligner(B);
            times_pending = false;
        }
        D.set_n += S.fresh;
        B->clock.mark(st, GS_ELF_PLAN);
        B->stats.ms_stage[ST_DEVICE_WAIT] += ms_since(th);  // (the host's wait for the iteration's GPU work)
        // host bookkeeping: the iteration's wall time less the aligner and the device waits
        B->stats.ms_host += ms_since(t_iter) - align_ms - (wait_ms - wait0);
        static const bool edbg = getenv("NPGX_ELF_DEBUG") != nullptr;
        if (edbg)
            fprintf(stderr, "elf(dev) it %d: ou_in %lld kept %lld state %016llx\n", it, (long long)S.ou_in,
                    (long long)S.nb, (unsigned long long)S.state);
        return !states.insert(S.state).second;
    }

    // OverlaplessUnion on the host (the multiset mode, or more conflicts than
    // the list holds): its input, the other table, comes down with the
    // MoveUnchanged flags, the result goes up as the current table, and the
    // plan is made again
    void ou_on_host() {
        deps_grow_if_full(D, S);
        B->stats.counters[CT_SPARE]++;  // (device loop: OverlaplessUnion runs the host took)
        std::vector<Block> v;
        dt_download(B, D, t ^ 1, S.nb1, S.nfr1, v, true);
        const std::vector<uint32_t> rank = extended_first_rank(v);
        bb::overlapless_union(B, v, &rank);  // (the host's, not the step above)
        for (Block& b : v) b.held = false;
        int64_t nb2 = 0, nfr2 = 0;
        dt_upload(B, D, t, v, nb2, nfr2);
        sum_upload(B, D, nb2, nfr2);
        plan(nb2);
    }

    // the loop's blocks back to the host
    void leave() {
        dt_download(B, D, t, S.nb, S.nfr, B->blocks, false);
        if (times_pending) collect_aligner(B);  // (the download waited for the last launch)
        B->clock.mark(st, GS_ELF_DOWNLOAD);
    }
};

// ExtendLoopFast's pipe on the device tables: MoveUnchanged and the flank plan
// (enter, then every tail) -> flank decode -> align -> stitch -> FixEnds and
// slicing -> OverlaplessUnion -> the Pipe's state check (tail)
static void extend_loop_fast_dev_run(npgx_blockset* B, ElfEntry& E, int64_t pre_nb, int64_t pre_nfr) {
    ElfLoop L(B, E);
    L.enter(pre_nb, pre_nfr);
    for (int it = 0; it < B->opt.max_iterations || B->opt.max_iterations == -1; it++) {
        L.decode_flanks(it);
        L.align();
        L.stitch();
        L.fix_ends();
        L.overlapless_union();
        if (L.tail()) break;
    }
    L.leave();
}

// pre_nb >= 0: table 0 already holds pre_nb blocks / pre_nfr fragments with
// their rows in arena[cur] (anchors_to_device); B->blocks is empty then, and
// stays empty on a failure
static void extend_loop_fast_dev(npgx_blockset* B, int64_t pre_nb = -1, int64_t pre_nfr = 0) {
    ElfEntry E{B->cur, B->used, false};
    try {
        extend_loop_fast_dev_run(B, E, pre_nb, pre_nfr);
    } catch (...) {
        // the set keeps its blocks as they came in; the aligner's word tables
        // are cleared before its next launch (launches already enqueued may
        // have used epochs the host never heard back about)
        if (E.swapped) B->arena[E.cur].swap(B->arena_x);
        B->cur = E.cur;
        B->used = E.used;
        aligner_note_epoch(B->aligner, 0xF000);
        throw;
    }
}

// OverlaplessUnion --ou-move of B->blocks through the device path (the
// engine processor "OverlaplessUnion@device", for parity tests on arbitrary
// blocks; inputs outside the device rules go to the host as in the loop).
// Names must all be the null name.  Returns true if the device decided.
static bool overlapless_union_dev(npgx_blockset* B) {
    for (const Block& b : B->blocks)
        NPGX_REQUIRE(b.name == NULL_BLOCK_NAME, NPGX_ERR_ARG, "OverlaplessUnion@device: named blocks");
    ElfDev& D = elf_dev(B);
    hipStream_t st = B->stream;
    elf_static(B, D);
    int64_t nb = 0, nfr = 0;
    dt_upload(B, D, 0, B->blocks, nb, nfr, true);
    sum_upload(B, D, nb, nfr, true);
    dt_ou_launch(B, D, 0, nb, nfr);
    ElfSum* out = (ElfSum*)B->pinned.take(sizeof(ElfSum), st);
    NPGX_HIP(hipMemcpyAsync(out, D.sum.p, sizeof(ElfSum), hipMemcpyDeviceToHost, st));
    sync(B);
    const ElfSum S = *out;
    if (S.flags & (ES_OU_HOST | ES_OU_CAP)) {
        deps_grow_if_full(D, S);
        overlapless_union(B, B->blocks);
        return false;
    }
    B->stats.counters[CT_OU_IN] += S.ou_in;
    B->stats.counters[CT_OU_REJECTED] += S.ou_rej;
    dt_download(B, D, 1, S.nb, S.nfr, B->blocks, false);
    return true;
}

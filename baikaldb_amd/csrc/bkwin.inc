// bkwin.inc — WindowNode for gfx950, included into bkgpu.hip.
//
// Re-creates the reference's WindowNode + WindowFnCall: NON-FRAME mode
// (src/exec/window_node.cpp:39-41: no frame / UNBOUNDED-UNBOUNDED both run
// the NonFrameWindowProcessor — every fn sees its whole partition;
// src/expr/window_fn_call.cpp:364-700 call/get_result semantics) and the
// ROWS / RANGE frames of BkFrameMode (window_node.cpp:49-58).
//
// MI355X shape: the input is fully sorted by (partition, order keys,
// arrival) — the existing top-N selector with limit = all passing rows IS
// that sort (LSD radix over order-preserving encodings). Window evaluation
// is then four steps over the sorted row ids:
//   1. k_win_flags : partition-change + peer-change flags (MemRowCompare
//      equality: NULLs compare equal, mem_row_compare.cpp:18-40)
//   2. rocprim scans: partition ids (sum), peer-group heads (max of
//      (partid<<40|pos), valid while n < 2^40 and np < 2^24 — the monotone
//      partition id in the high bits makes a global max-scan segment-local),
//      cumulative peer-change counts (dense rank)
//   3. k_win_agg : per-thread-slice segmented reduction of the aggregate
//      fns (atomic merges only at slice/partition boundaries — never
//      per-row, which would hit the ~20 G ops/s memory-side atomic wall)
//   4. k_win_emit: every fn's value per row from the scan arrays + the
//      per-partition states.
// A frame adds, between 3 and 4, what its aggregates read: global prefix
// sums and counts (k_win_frame_vals + scans), a sparse table for MIN/MAX
// (k_win_st_base/level) and, for RANGE by value, the order-key encodings
// (k_win_ordenc). win_frame_bounds is the only place that knows what a
// frame mode means; the host stages at the end of the file run in the order
// above.

/* the sorted stream and the partition/peer structure over it (host stage
 * win_structure fills it, k_win_emit reads it) */
struct WinStream {
    int64_t*  rowid;     /* [n] global row ids in (partition, order, arrival) order */
    uint32_t* partid1;   /* [n] 1-based partition id */
    uint64_t* peerB;     /* [n] low 40 bits: position of the row's peer-group head */
    uint64_t* peerC;     /* [n] cumulative peer-change count = global peer-group id */
    uint64_t* peer_end;  /* [peer-group id] one past the group's last position */
    int64_t*  bounds;    /* [np + 1] partition start positions, bounds[np] = n */
    uint64_t* states;    /* [np][nfns] {u64 val, u64 cnt} whole-partition aggregates */
    int64_t   n;
};

struct WinFrame {
    int32_t mode;             /* BkFrameMode */
    int32_t ord_col;          /* first order key, -1 without one */
    int32_t ord_null_first;
    int64_t pre, fol;         /* ROWS / RANGE_VALUE bounds, negative = UNBOUNDED */
};

/* what frame aggregates read; a pointer stays null in the modes and fn
 * mixes that never dereference it */
struct WinFrameIn {
    uint64_t* FS;        /* [f][n] inclusive prefix sums (u64 wrap or f64 bits) */
    uint64_t* FC;        /* [f][n] inclusive prefix non-null counts */
    uint64_t* ST;        /* [level][f][n] MIN/MAX sparse table */
    uint64_t* ENCo;      /* [n] order-key encodings (BK_FRAME_RANGE_VALUE) */
    int32_t   st_levels;
};

/* fn-major outputs [f*n + i] */
struct WinOut {
    int64_t* out_i;
    double*  out_d;
    uint8_t* out_null;
};

struct WinCompareCols {
    int32_t n_part;     /* 0 = single whole-set partition */
    int32_t part[3];    /* PARTITION BY columns (window_node.cpp evaluates
                           all partition exprs per row; a new partition
                           starts when ANY of them changes) */
    int32_t n_ord;
    int32_t ord[4];
};

/* value equality per MemRowCompare: NULLs equal each other */
__device__ __forceinline__ bool win_cell_eq(const DevCol& c, int64_t ra,
                                            int64_t rb) {
    bool va = cell_valid(c, ra), vb = cell_valid(c, rb);
    if (va != vb) return false;
    if (!va) return true;
    return enc_value(c, ra) == enc_value(c, rb);
}

__global__ void k_win_flags(DevCols cols, WinCompareCols w,
                            const int64_t* rowid, int64_t n,
                            uint32_t* segf, uint32_t* peerf) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs) {
        uint32_t s = 0, p = 0;
        if (i == 0) {
            s = p = 1;
        } else {
            for (int k = 0; k < w.n_part && !s; k++)
                if (!win_cell_eq(cols.c[w.part[k]], rowid[i], rowid[i - 1]))
                    s = 1;
            p = s;
            if (!p) {
                for (int k = 0; k < w.n_ord; k++) {
                    if (!win_cell_eq(cols.c[w.ord[k]], rowid[i], rowid[i - 1])) {
                        p = 1;
                        break;
                    }
                }
            }
        }
        segf[i] = s;
        peerf[i] = p;
    }
}

/* B[i] for the peer-head max-scan (see header comment) */
__global__ void k_win_peerpos(const uint32_t* partid1, const uint32_t* peerf,
                              int64_t n, uint64_t* B) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs)
        B[i] = ((uint64_t)partid1[i] << 40) | (peerf[i] ? (uint64_t)i : 0);
}

/* per-peer-group end positions: peer groups are numbered globally by the
 * cumulative peer-change count (peerC); group g ends after max(i)+1 */
__global__ void k_win_peerend(const uint64_t* peerC, int64_t n,
                              uint64_t* peer_end) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs)
        atomicMax((unsigned long long*)&peer_end[peerC[i]],
                  (unsigned long long)(i + 1));
}

/* partition bounds: bounds[partid1[i]-1] = i at each segment head */
__global__ void k_win_bounds(const uint32_t* partid1, const uint32_t* segf,
                             int64_t n, int64_t* bounds, int64_t np) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs)
        if (segf[i]) bounds[partid1[i] - 1] = i;
    if (blockIdx.x == 0 && threadIdx.x == 0) bounds[np] = n;
}

/* per-partition aggregate states: [p][f] = {u64 val, u64 cnt}.
 * Each thread owns a CONTIGUOUS slice of rows and merges its private
 * accumulators into the global state only when its run's partition ends. */
__global__ void k_win_agg(DevCols cols, const int64_t* rowid,
                          const uint32_t* partid1, int64_t n, int64_t rows_per,
                          uint64_t* states, const BkWindowFn* fns, int nfns) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t i0 = t * rows_per;
    if (i0 >= n) return;
    int64_t i1 = i0 + rows_per < n ? i0 + rows_per : n;
    /* accumulators for up to BK_MAX_WINFNS fns; indexed by the run-time fn
     * number, so they live in per-lane scratch (80 B), not in registers */
    uint64_t av[BK_MAX_WINFNS];
    uint64_t ac[BK_MAX_WINFNS];
    double ad[BK_MAX_WINFNS];
    uint32_t cur = partid1[i0];
    #pragma unroll
    for (int f = 0; f < BK_MAX_WINFNS; f++) { av[f] = 0; ac[f] = 0; ad[f] = 0; }
    auto flush = [&](uint32_t p1) {
        uint64_t* st = states + ((size_t)(p1 - 1) * nfns) * 2;
        for (int f = 0; f < nfns; f++) {
            int ft = fns[f].fn_type;
            uint64_t* val = st + 2 * f;
            uint64_t* cnt = val + 1;
            switch (ft) {
                case BK_WIN_COUNT_STAR:
                case BK_WIN_COUNT:
                    if (ac[f]) atomicAdd((unsigned long long*)cnt,
                                         (unsigned long long)ac[f]);
                    break;
                case BK_WIN_SUM:
                case BK_WIN_AVG:
                    if (ac[f]) {
                        if (cols.c[fns[f].col].type == BK_DOUBLE ||
                            ft == BK_WIN_AVG)
                            atomic_add_f64_global(val, ad[f]);
                        else
                            atomicAdd((unsigned long long*)val,
                                      (unsigned long long)av[f]);
                        atomicAdd((unsigned long long*)cnt,
                                  (unsigned long long)ac[f]);
                    }
                    break;
                case BK_WIN_MIN:
                case BK_WIN_MAX:
                    if (ac[f]) {
                        atomicMax((unsigned long long*)val,
                                  (unsigned long long)av[f]);
                        atomicAdd((unsigned long long*)cnt,
                                  (unsigned long long)ac[f]);
                    }
                    break;
                default: break;
            }
        }
        for (int f = 0; f < nfns; f++) { av[f] = 0; ac[f] = 0; ad[f] = 0; }
    };
    for (int64_t i = i0; i < i1; i++) {
        uint32_t p1 = partid1[i];
        if (p1 != cur) { flush(cur); cur = p1; }
        int64_t r = rowid[i];
        for (int f = 0; f < nfns; f++) {
            int ft = fns[f].fn_type;
            if (ft == BK_WIN_COUNT_STAR) { ac[f]++; continue; }
            if (ft > BK_WIN_MAX) continue;   /* rank/value fns: no state */
            const DevCol& c = cols.c[fns[f].col];
            if (!cell_valid(c, r)) continue;
            switch (ft) {
                case BK_WIN_COUNT: ac[f]++; break;
                case BK_WIN_SUM:
                    if (c.type == BK_DOUBLE) ad[f] += ((const double*)c.data)[r];
                    else av[f] += (uint64_t)cell_i64(c, r);
                    ac[f]++;
                    break;
                case BK_WIN_AVG: ad[f] += cell_f64(c, r); ac[f]++; break;
                case BK_WIN_MIN: {
                    uint64_t e = ~enc_value(c, r);
                    if (!ac[f] || e > av[f]) av[f] = e;
                    ac[f]++;
                    break;
                }
                case BK_WIN_MAX: {
                    uint64_t e = enc_value(c, r);
                    if (!ac[f] || e > av[f]) av[f] = e;
                    ac[f]++;
                    break;
                }
                default: break;
            }
        }
    }
    flush(cur);
}

/* ROWS-frame support (RowFrameWindowProcessor, window_node.cpp:49-58):
 * per frame-aggregate fn, GLOBAL inclusive prefix arrays over the sorted
 * stream — sum (u64 wrap for int64 inputs = reference modular adds; f64 for
 * double/avg) and non-null count. A frame [l,r] clamped inside the partition
 * then evaluates as prefix differences; partitions need no segmenting
 * because l,r never cross them. */
__global__ void k_win_frame_vals(DevCols cols, const int64_t* rowid,
                                 const BkWindowFn* fns, int nfns, int64_t n,
                                 uint64_t* S, uint64_t* Cc) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs) {
        int64_t r = rowid[i];
        for (int f = 0; f < nfns; f++) {
            int ft = fns[f].fn_type;
            int64_t idx = (int64_t)f * n + i;
            if (ft == BK_WIN_COUNT_STAR) { S[idx] = 0; Cc[idx] = 1; continue; }
            if (ft > BK_WIN_MAX || ft < BK_WIN_COUNT) { S[idx] = 0; Cc[idx] = 0; continue; }
            const DevCol& c = cols.c[fns[f].col];
            if (!cell_valid(c, r)) { S[idx] = 0; Cc[idx] = 0; continue; }
            Cc[idx] = 1;
            if (ft == BK_WIN_COUNT || ft == BK_WIN_MIN || ft == BK_WIN_MAX) {
                S[idx] = 0;
                continue;
            }
            if (c.type == BK_DOUBLE || ft == BK_WIN_AVG) {
                double d = cell_f64(c, r);
                memcpy(&S[idx], &d, 8);
            } else {
                S[idx] = (uint64_t)cell_i64(c, r);
            }
        }
    }
}

/* frame MIN/MAX: a sparse table over the order-encoded values of the
 * sorted stream (NULLs contribute the identity 0 — encodings of valid
 * values are handled as unsigned max; MIN uses the complement, exactly the
 * aggregate-state trick of DESIGN §2). Level k holds the max over
 * [i, i+2^k); a frame [l, r] is the max of two overlapping spans. Build is
 * log2(n) cheap passes; query O(1). */
__global__ void k_win_st_base(DevCols cols, const int64_t* rowid,
                              const BkWindowFn* fns, int nfns, int64_t n,
                              uint64_t* st /* [f][n] level 0 */) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs) {
        int64_t r = rowid[i];
        for (int f = 0; f < nfns; f++) {
            int ft = fns[f].fn_type;
            if (ft != BK_WIN_MIN && ft != BK_WIN_MAX) continue;
            const DevCol& c = cols.c[fns[f].col];
            uint64_t e = 0;   /* NULL rows contribute the max-identity 0;
                                 emptiness is detected via the frame COUNT
                                 prefix (FC), not the value */
            if (cell_valid(c, r)) {
                e = enc_value(c, r);
                if (ft == BK_WIN_MIN) e = ~e;
            }
            st[(size_t)f * n + i] = e;
        }
    }
}

__global__ void k_win_st_level(const uint64_t* prev, uint64_t* cur,
                               int64_t n, int64_t span, int nfns) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    int64_t total = (int64_t)nfns * n;
    for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total;
         x += gs) {
        int64_t i = x % n;
        int64_t j = i + span;
        uint64_t a = prev[x];
        if (j < n) {
            uint64_t b = prev[x - i + j];
            a = b > a ? b : a;
        }
        cur[x] = a;
    }
}

/* RANGE value-offset frames (mode 4): the order-key encodings of the
 * sorted stream, for per-row binary search of [v-pre, v+fol]. NULL-key
 * rows get 0 (they are excluded by the non-null span bounds). */
__global__ void k_win_ordenc(DevCols cols, int ord_col, const int64_t* rowid,
                             int64_t n, uint64_t* enc) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    const DevCol& c = cols.c[ord_col];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs)
        enc[i] = cell_valid(c, rowid[i]) ? enc_value(c, rowid[i]) : 0;
}

/* ---- k_win_emit and its pieces: one frame resolver, one evaluator per fn
 * family, one ENC decode ---- */

/* inclusive span [fl, fr] of sorted positions; empty when fr < fl */
struct WinSpan { int64_t fl, fr; };

__device__ __forceinline__ int64_t win_peer_head(const WinStream& s, int64_t i) {
    return (int64_t)(s.peerB[i] & 0xFFFFFFFFFFull);
}
/* one past the last position of i's peer group */
__device__ __forceinline__ int64_t win_peer_end(const WinStream& s, int64_t i) {
    return (int64_t)s.peer_end[s.peerC[i]];
}

/* first position in [lo, hi) whose order-key encoding is not below t
 * (incl: not below-or-equal), the span's encodings being ascending */
__device__ __forceinline__ int64_t win_enc_search(const uint64_t* ENCo, int64_t lo,
                                                  int64_t hi, uint64_t t, bool incl) {
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if (incl ? ENCo[mid] <= t : ENCo[mid] < t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

/* THE definition of the five frame modes: the frame of row i, clamped to its
 * partition [ps, pe). */
__device__ __forceinline__ WinSpan win_frame_bounds(
        const DevCols& cols, const WinStream& s, const WinFrame& fm,
        const uint64_t* ENCo, int64_t i, int64_t ps, int64_t pe,
        int64_t peer_head) {
    WinSpan w{ps, pe - 1};   /* BK_FRAME_NONE: the whole partition */
    if (fm.mode == BK_FRAME_ROWS) {
        /* ROWS [i-pre, i+fol], negative bound = UNBOUNDED */
        if (fm.pre >= 0) w.fl = i - fm.pre > ps ? i - fm.pre : ps;
        if (fm.fol >= 0) w.fr = i + fm.fol < pe - 1 ? i + fm.fol : pe - 1;
    } else if (fm.mode == BK_FRAME_RANGE_UPC) {
        /* RANGE UNBOUNDED PRECEDING..CURRENT ROW = [ps, end of current peer
         * group) */
        w.fr = win_peer_end(s, i) - 1;
    } else if (fm.mode == BK_FRAME_RANGE_CRF) {
        /* RANGE CURRENT ROW..UNBOUNDED FOLLOWING = [peer head, pe) */
        w.fl = peer_head;
    } else if (fm.mode == BK_FRAME_RANGE_VALUE) {
        /* RANGE BETWEEN pre PRECEDING AND fol FOLLOWING by VALUE over the
         * single ASC integer order key (negative bound = UNBOUNDED).
         * NULL-key rows frame their own peer group (NULLs are peers);
         * non-null rows binary-search the partition's non-null span over
         * the order-key encodings. */
        const DevCol& oc = cols.c[fm.ord_col];
        if (oc.valid && !cell_valid(oc, s.rowid[i])) {
            w.fl = peer_head;
            w.fr = win_peer_end(s, i) - 1;
        } else {
            int64_t nn_lo = ps, nn_hi = pe;
            if (oc.valid) {
                if (fm.ord_null_first) {
                    if (!cell_valid(oc, s.rowid[ps])) nn_lo = win_peer_end(s, ps);
                } else {
                    if (!cell_valid(oc, s.rowid[pe - 1]))
                        nn_hi = win_peer_head(s, pe - 1);
                }
            }
            uint64_t v = ENCo[i];
            if (fm.pre < 0) {
                w.fl = nn_lo;
            } else {
                uint64_t lo_t = v >= (uint64_t)fm.pre ? v - (uint64_t)fm.pre : 0;
                w.fl = win_enc_search(ENCo, nn_lo, i, lo_t, false);
            }
            if (fm.fol < 0) {
                w.fr = nn_hi - 1;
            } else {
                uint64_t hi_t = v + (uint64_t)fm.fol >= v ? v + (uint64_t)fm.fol
                                                          : ~0ull;
                w.fr = win_enc_search(ENCo, i, nn_hi, hi_t, true) - 1;
            }
        }
    }
    return w;
}

/* one output value: loads input col at sorted position j (global row
 * rowid[j]); writes typed out + null flag */
__device__ __forceinline__ void win_emit_value(const DevCols& cols, int col,
                                               const int64_t* rowid, int64_t j,
                                               int64_t idx, const WinOut& o) {
    const DevCol& c = cols.c[col];
    int64_t r = rowid[j];
    if (!cell_valid(c, r)) { o.out_null[idx] = 1; return; }
    o.out_null[idx] = 0;
    if (c.type == BK_DOUBLE) o.out_d[idx] = ((const double*)c.data)[r];
    else o.out_i[idx] = cell_i64(c, r);
}

/* the one ENC -> typed output decode of a MIN/MAX result (MIN states hold
 * the complement) */
__device__ __forceinline__ void win_store_enc(const DevCol& c, uint64_t e,
                                              bool is_min, int64_t idx,
                                              const WinOut& o) {
    if (is_min) e = ~e;
    if (c.type == BK_DOUBLE) o.out_d[idx] = bk_dec_f64(e);
    else if (c.type == BK_STRING) o.out_i[idx] = (int64_t)(uint32_t)e;
    else o.out_i[idx] = bk_dec_i64(e);
}

/* non-null rows of fn f inside the frame, from its COUNT prefix Cf; an empty
 * frame counts 0, so "no value => NULL" is one rule for every aggregate */
__device__ __forceinline__ uint64_t win_frame_count(const uint64_t* Cf, WinSpan w) {
    if (w.fr < w.fl) return 0;
    return Cf[w.fr] - (w.fl > 0 ? Cf[w.fl - 1] : 0);
}

/* frame MIN/MAX of a frame with a value: max of two overlapping sparse-table
 * spans of level k = floor(log2(len)) */
__device__ __forceinline__ void win_frame_minmax(const DevCol& c, bool is_min,
                                                 const WinFrameIn& in, int f,
                                                 int nfns, int64_t n, WinSpan w,
                                                 int64_t idx, const WinOut& o) {
    int64_t len = w.fr - w.fl + 1;
    int k = 63 - __clzll((unsigned long long)len);
    if (k >= in.st_levels) k = in.st_levels - 1;
    const uint64_t* Lk = in.ST + ((size_t)k * nfns + f) * n;
    uint64_t a = Lk[w.fl];
    uint64_t b = Lk[w.fr - (1ll << k) + 1];
    win_store_enc(c, a > b ? a : b, is_min, idx, o);
}

/* frame SUM/AVG of a frame with fcnt > 0 values, from the prefix sums Sf */
__device__ __forceinline__ void win_frame_sum(const DevCol& c, bool avg,
                                              const int64_t* rowid,
                                              const uint64_t* Sf, uint64_t fcnt,
                                              WinSpan w, int64_t idx,
                                              const WinOut& o) {
    if (c.type != BK_DOUBLE && !avg) {
        o.out_i[idx] = (int64_t)(Sf[w.fr] - (w.fl > 0 ? Sf[w.fl - 1] : 0));
        return;
    }
    double sum;
    if (w.fr - w.fl < 64) {
        /* SHORT frames sum directly in frame order — the
         * reference accumulates per frame (ExprValue::add
         * sequence), so its error is ~ulp(frame sum); a
         * prefix DIFFERENCE carries ~ulp(prefix total),
         * which at 2^40-scale int64 inputs over 2e4 rows
         * exceeds the documented 1e-10 tolerance (observed
         * |err| 2.5 on a 2-row AVG frame). */
        sum = 0.0;
        for (int64_t j = w.fl; j <= w.fr; j++) {
            int64_t r = rowid[j];
            if (cell_valid(c, r)) sum += cell_f64(c, r);
        }
    } else {
        double hi, lo = 0.0;
        memcpy(&hi, &Sf[w.fr], 8);
        if (w.fl > 0) memcpy(&lo, &Sf[w.fl - 1], 8);
        sum = hi - lo;
    }
    o.out_d[idx] = avg ? sum / (double)fcnt : sum;
}

/* whole-partition aggregate from the k_win_agg state {val, cnt} */
__device__ __forceinline__ void win_part_agg(const DevCols& cols,
                                             const BkWindowFn& fn, uint64_t val,
                                             uint64_t cnt, int64_t idx,
                                             const WinOut& o) {
    int ft = fn.fn_type;
    if (ft == BK_WIN_COUNT_STAR || ft == BK_WIN_COUNT) {
        o.out_i[idx] = (int64_t)cnt;
        return;
    }
    if (!cnt) { o.out_null[idx] = 1; return; }
    const DevCol& c = cols.c[fn.col];
    if (ft == BK_WIN_MIN || ft == BK_WIN_MAX) {
        win_store_enc(c, val, ft == BK_WIN_MIN, idx, o);
    } else if (ft == BK_WIN_AVG || c.type == BK_DOUBLE) {
        double d; memcpy(&d, &val, 8);
        o.out_d[idx] = ft == BK_WIN_AVG ? d / (double)cnt : d;
    } else {
        o.out_i[idx] = (int64_t)val;
    }
}

__global__ void k_win_emit(DevCols cols, WinStream s, WinFrame fm, WinFrameIn in,
                           const BkWindowFn* fns, int nfns, WinOut o) {
    int64_t n = s.n;
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs) {
        uint32_t p1 = s.partid1[i];
        int64_t ps = s.bounds[p1 - 1], pe = s.bounds[p1];
        int64_t pn = pe - ps;
        int64_t peer_head = win_peer_head(s, i);
        const uint64_t* st = s.states + ((size_t)(p1 - 1) * nfns) * 2;
        WinSpan w = win_frame_bounds(cols, s, fm, in.ENCo, i, ps, pe, peer_head);
        for (int f = 0; f < nfns; f++) {
            int ft = fns[f].fn_type;
            int64_t idx = (int64_t)f * n + i;
            o.out_i[idx] = 0; o.out_d[idx] = 0.0; o.out_null[idx] = 0;
            bool minmax = ft == BK_WIN_MIN || ft == BK_WIN_MAX;
            if (fm.mode != BK_FRAME_NONE && (minmax || ft <= BK_WIN_AVG)) {
                /* frame aggregates from the prefix arrays / sparse table */
                uint64_t fcnt = win_frame_count(in.FC + (size_t)f * n, w);
                if (ft == BK_WIN_COUNT_STAR || ft == BK_WIN_COUNT)
                    o.out_i[idx] = (int64_t)fcnt;
                else if (!fcnt)   /* empty frame or all NULL */
                    o.out_null[idx] = 1;
                else if (minmax)
                    win_frame_minmax(cols.c[fns[f].col], ft == BK_WIN_MIN, in,
                                     f, nfns, n, w, idx, o);
                else
                    win_frame_sum(cols.c[fns[f].col], ft == BK_WIN_AVG, s.rowid,
                                  in.FS + (size_t)f * n, fcnt, w, idx, o);
                continue;
            }
            switch (ft) {
                case BK_WIN_COUNT_STAR: case BK_WIN_COUNT: case BK_WIN_SUM:
                case BK_WIN_AVG: case BK_WIN_MIN: case BK_WIN_MAX:
                    win_part_agg(cols, fns[f], st[2 * f], st[2 * f + 1], idx, o);
                    break;
                case BK_WIN_ROW_NUMBER: o.out_i[idx] = i - ps + 1; break;
                case BK_WIN_RANK: o.out_i[idx] = peer_head - ps + 1; break;
                case BK_WIN_DENSE_RANK:
                    o.out_i[idx] = (int64_t)(s.peerC[i] - s.peerC[ps]) + 1;
                    break;
                case BK_WIN_PERCENT_RANK:
                    /* (rank-1)/(n-1); 0 for single-row partitions
                     * (window_fn_call.cpp:570-607) */
                    o.out_d[idx] = pn > 1
                        ? (double)(peer_head - ps) / (double)(pn - 1) : 0.0;
                    break;
                case BK_WIN_FIRST_VALUE:
                case BK_WIN_LAST_VALUE:
                case BK_WIN_NTH_VALUE: {
                    /* a position of the frame, NULL when it is not inside */
                    int64_t j = ft == BK_WIN_FIRST_VALUE ? w.fl
                              : ft == BK_WIN_LAST_VALUE ? w.fr
                              : w.fl + fns[f].param - 1;
                    if (j >= w.fl && j <= w.fr)
                        win_emit_value(cols, fns[f].col, s.rowid, j, idx, o);
                    else o.out_null[idx] = 1;
                    break;
                }
                case BK_WIN_LEAD:
                case BK_WIN_LAG: {
                    int64_t off = fns[f].param > 0 ? fns[f].param : 1;
                    int64_t j = ft == BK_WIN_LEAD ? i + off : i - off;
                    if (j >= ps && j < pe) {
                        win_emit_value(cols, fns[f].col, s.rowid, j, idx, o);
                    } else if (fns[f].has_def) {
                        if (cols.c[fns[f].col].type == BK_DOUBLE)
                            o.out_d[idx] = fns[f].def_d;
                        else o.out_i[idx] = fns[f].def_i;
                    } else {
                        o.out_null[idx] = 1;
                    }
                    break;
                }
                case BK_WIN_CUME_DIST:
                    /* rows <= current peer group / partition rows
                     * (window_fn_call.cpp:609-655) */
                    o.out_d[idx] = (double)(win_peer_end(s, i) - ps) / (double)pn;
                    break;
                case BK_WIN_NTILE: {
                    /* first `rem` buckets take quot+1 rows
                     * (window_fn_call.cpp:456-467, NTILE get_result) */
                    int64_t k = fns[f].param > 0 ? fns[f].param : 1;
                    int64_t quot = pn / k, rem = pn % k;
                    int64_t j = i - ps;
                    int64_t fat = rem * (quot + 1);
                    o.out_i[idx] = j < fat
                        ? j / (quot + 1) + 1
                        : rem + (quot > 0 ? (j - fat) / quot : 0) + 1;
                    break;
                }
                default: o.out_null[idx] = 1; break;
            }
        }
    }
}

/* ---- host: the window pipeline as stages, in the order they run. A stage
 * returns <0 with g_err set on failure; its device buffers belong to the
 * caller's PoolBufs. ---- */

#define WIN_TRY(expr) BK_TRY("window", expr, -1)
/* every window kernel is a grid-stride loop launched 2048 x 256 */
#define WIN_LAUNCH(k, ...) \
    hipLaunchKernelGGL(k, dim3(2048), dim3(256), 0, 0, __VA_ARGS__)

/* the fn list: host copy for planning, device copy for the kernels */
struct WinFns {
    const BkWindowFn* h;
    BkWindowFn* d;
    int n;
};

/* fns that read an input column (the others carry col = -1) */
static bool win_fn_reads_col(int ft) {
    switch (ft) {
        case BK_WIN_COUNT_STAR: case BK_WIN_ROW_NUMBER: case BK_WIN_RANK:
        case BK_WIN_DENSE_RANK: case BK_WIN_PERCENT_RANK:
        case BK_WIN_CUME_DIST: case BK_WIN_NTILE:
            return false;
        default:
            return true;
    }
}

static int win_check_args(const BkgTable* t, const int32_t* part_cols,
                          int32_t n_part, const BkOrderSpec* order, int norder,
                          const BkWindowFn* fns, int nfns, int32_t frame_mode) {
    if (nfns < 1 || nfns > BK_MAX_WINFNS) { set_err("window: bad nfns"); return -1; }
    if (norder < 0 || norder > 3) { set_err("window: bad norder"); return -1; }
    if (n_part < 0 || n_part > 3) { set_err("window: bad n_part"); return -1; }
    if (n_part + norder > 4) {
        set_err("window: n_part + norder > 4 sort keys");
        return -1;
    }
    for (int k = 0; k < n_part; k++)
        if (part_cols[k] < 0 || part_cols[k] >= t->ncols) {
            set_err("window: bad partition col");
            return -1;
        }
    if (frame_mode == BK_FRAME_RANGE_VALUE) {
        int oc = norder == 1 ? order[0].col : -1;
        int32_t octy = oc >= 0 ? t->specs[oc].col_type : -1;
        if (norder != 1 || !order[0].is_asc ||
            (octy != BK_INT64 && octy != BK_DATETIME)) {
            set_err("window: RANGE value frames need one ASC integer "
                    "order key");
            return -1;
        }
    }
    for (int f = 0; f < nfns; f++)
        if (win_fn_reads_col(fns[f].fn_type) &&
            (fns[f].col < 0 || fns[f].col >= t->ncols)) {
            set_err("window: bad fn col");
            return -1;
        }
    return 0;
}

/* full sort by (partition, order, arrival) via the top-N machinery with
 * limit = everything. Row ids land in out_rowids (host, part of the result)
 * and in s.rowid; returns rows passing q. */
static int64_t win_sort(PoolBufs& bufs, BkgTable* t, const BkQuerySpec* q,
                        const WinCompareCols& w, const BkOrderSpec* order,
                        int64_t row_begin, int64_t row_end,
                        int64_t* out_rowids, WinStream& s) {
    BkOrderSpec full[4];
    int nf = 0;
    for (int k = 0; k < w.n_part; k++) full[nf++] = {w.part[k], 1, 1, 0};
    for (int k = 0; k < w.n_ord && nf < 4; k++) full[nf++] = order[k];
    int64_t range = row_end - row_begin;
    int64_t n;
    if (nf == 0) {
        /* no partition, no order keys: output order = arrival order */
        n = bkgpu_filter_collect(t, q, row_begin, row_end, range, out_rowids);
        if (n > 0) std::sort(out_rowids, out_rowids + n);
    } else {
        n = bkgpu_sort_topk(t, q, full, nf, row_begin, row_end, range,
                            out_rowids);
    }
    if (n <= 0) return n;
    if (n >= (1ll << 40)) { set_err("window: too many rows"); return -1; }
    s.n = n;
    WIN_TRY(bufs.get(&s.rowid, (size_t)n * 8));
    /* the sort hands its ids to the host; a device-side hand-off needs
     * bkgpu_sort_topk split in two, so they go up again here */
    WIN_TRY(hipMemcpy(s.rowid, out_rowids, (size_t)n * 8, hipMemcpyHostToDevice));
    return n;
}

/* partition/peer structure of the sorted stream: flags, three scans,
 * bounds, whole-partition aggregate states, peer-group ends */
static int win_structure(PoolBufs& bufs, const DevCols& dc,
                         const WinCompareCols& w, const WinFns& fns,
                         WinStream& s) {
    const int64_t n = s.n;
    uint32_t *segf = nullptr, *peerf = nullptr;
    WIN_TRY(bufs.get(&segf, (size_t)n * 4));
    WIN_TRY(bufs.get(&peerf, (size_t)n * 4));
    WIN_TRY(bufs.get(&s.partid1, (size_t)n * 4));
    WIN_TRY(bufs.get(&s.peerB, (size_t)n * 8));
    WIN_TRY(bufs.get(&s.peerC, (size_t)n * 8));
    WIN_LAUNCH(k_win_flags, dc, w, s.rowid, n, segf, peerf);
    /* partition ids (1-based): inclusive sum scan of segf */
    WIN_TRY(dev_inclusive_scan(bufs, segf, s.partid1, (size_t)n, DevPlus<uint32_t>()));
    WIN_TRY(dev_inclusive_scan(bufs, peerf, s.peerC, (size_t)n, DevPlus<uint64_t>()));
    WIN_LAUNCH(k_win_peerpos, s.partid1, peerf, n, s.peerB);
    WIN_TRY(dev_inclusive_scan(bufs, s.peerB, s.peerB, (size_t)n, DevMax<uint64_t>()));
    uint32_t np = 0;
    WIN_TRY(hipMemcpy(&np, s.partid1 + (n - 1), 4, hipMemcpyDeviceToHost));
    if (np >= (1u << 24)) { set_err("window: too many partitions"); return -1; }
    WIN_TRY(bufs.get(&s.bounds, ((size_t)np + 1) * 8));
    WIN_LAUNCH(k_win_bounds, s.partid1, segf, n, s.bounds, (int64_t)np);
    WIN_TRY(bufs.get(&s.states, (size_t)np * fns.n * 2 * 8));
    WIN_TRY(hipMemset(s.states, 0, (size_t)np * fns.n * 2 * 8));
    bool any_agg = false;
    for (int f = 0; f < fns.n; f++) any_agg |= fns.h[f].fn_type <= BK_WIN_MAX;
    if (any_agg) {
        int64_t total_threads = (int64_t)2048 * 256;
        int64_t rows_per = (n + total_threads - 1) / total_threads;
        WIN_LAUNCH(k_win_agg, dc, s.rowid, s.partid1, n, rows_per, s.states,
                   fns.d, fns.n);
    }
    uint64_t total_peers = 0;
    WIN_TRY(hipMemcpy(&total_peers, s.peerC + (n - 1), 8, hipMemcpyDeviceToHost));
    WIN_TRY(bufs.get(&s.peer_end, (total_peers + 1) * 8));
    WIN_TRY(hipMemset(s.peer_end, 0, (total_peers + 1) * 8));
    WIN_LAUNCH(k_win_peerend, s.peerC, n, s.peer_end);
    return 0;
}

/* frames: per aggregate fn the inclusive prefix counts, and the prefix sums
 * where the fn sums */
static int win_frame_prefixes(PoolBufs& bufs, const BkgTable* t,
                              const DevCols& dc, const WinStream& s,
                              const WinFns& fns, WinFrameIn& in) {
    const int64_t n = s.n;
    WIN_TRY(bufs.get(&in.FS, (size_t)fns.n * n * 8));
    WIN_TRY(bufs.get(&in.FC, (size_t)fns.n * n * 8));
    WIN_LAUNCH(k_win_frame_vals, dc, s.rowid, fns.d, fns.n, n, in.FS, in.FC);
    for (int f = 0; f < fns.n; f++) {
        int ft = fns.h[f].fn_type;
        if (ft > BK_WIN_MAX) continue;
        uint64_t* Sf = in.FS + (size_t)f * n;
        uint64_t* Cf = in.FC + (size_t)f * n;
        WIN_TRY(dev_inclusive_scan(bufs, Cf, Cf, (size_t)n, DevPlus<uint64_t>()));
        if (ft == BK_WIN_MIN || ft == BK_WIN_MAX || ft == BK_WIN_COUNT ||
            ft == BK_WIN_COUNT_STAR)
            continue;   /* counts only */
        bool dbl = ft == BK_WIN_AVG ||
                   (fns.h[f].col >= 0 &&
                    t->specs[fns.h[f].col].col_type == BK_DOUBLE);
        if (dbl)
            WIN_TRY(dev_inclusive_scan(bufs, (double*)Sf, (double*)Sf, (size_t)n,
                                       DevPlus<double>()));
        else
            WIN_TRY(dev_inclusive_scan(bufs, Sf, Sf, (size_t)n, DevPlus<uint64_t>()));
    }
    return 0;
}

/* frames with a MIN/MAX fn: the sparse table, levels sized by the max frame
 * length (bounded ROWS frames need only log2(pre+fol+1)+1 levels) */
static int win_sparse_table(PoolBufs& bufs, const DevCols& dc,
                            const WinStream& s, const WinFrame& fm,
                            const WinFns& fns, WinFrameIn& in) {
    bool frame_minmax = false;
    for (int f = 0; f < fns.n; f++)
        frame_minmax |= fns.h[f].fn_type == BK_WIN_MIN ||
                        fns.h[f].fn_type == BK_WIN_MAX;
    if (!frame_minmax) return 0;
    const int64_t n = s.n;
    int64_t maxlen = n;
    if (fm.mode == BK_FRAME_ROWS && fm.pre >= 0 && fm.fol >= 0)
        maxlen = fm.pre + fm.fol + 1;
    if (maxlen > n) maxlen = n;
    int levels = 1;
    while ((1ll << levels) < maxlen && levels < 40) levels++;
    levels += (1ll << (levels - 1)) < maxlen ? 1 : 0;
    size_t st_bytes = (size_t)levels * fns.n * (size_t)n * 8;
    if (st_bytes > (size_t)8 << 30) {
        set_err("window: frame MIN/MAX sparse table would exceed 8 GB "
                "(bound the frame or reduce rows)");
        return -1;
    }
    WIN_TRY(bufs.get(&in.ST, st_bytes));
    in.st_levels = levels;
    WIN_LAUNCH(k_win_st_base, dc, s.rowid, fns.d, fns.n, n, in.ST);
    for (int k = 1; k < levels; k++)
        WIN_LAUNCH(k_win_st_level, in.ST + ((size_t)(k - 1) * fns.n) * n,
                   in.ST + ((size_t)k * fns.n) * n, n, (int64_t)1 << (k - 1),
                   fns.n);
    return 0;
}

/* the order-key encodings where the frame searches them, then every fn's
 * value per row, then the download */
static int win_emit_download(PoolBufs& bufs, const DevCols& dc,
                             const WinStream& s, const WinFrame& fm,
                             WinFrameIn& in, const WinFns& fns, int64_t* out_i,
                             double* out_d, uint8_t* out_null) {
    const int64_t n = s.n;
    if (fm.mode == BK_FRAME_RANGE_VALUE) {
        WIN_TRY(bufs.get(&in.ENCo, (size_t)n * 8));
        WIN_LAUNCH(k_win_ordenc, dc, fm.ord_col, s.rowid, n, in.ENCo);
    }
    WinOut o{};
    WIN_TRY(bufs.get(&o.out_i, (size_t)fns.n * n * 8));
    WIN_TRY(bufs.get(&o.out_d, (size_t)fns.n * n * 8));
    WIN_TRY(bufs.get(&o.out_null, (size_t)fns.n * n));
    WIN_LAUNCH(k_win_emit, dc, s, fm, in, fns.d, fns.n, o);
    WIN_TRY(hipGetLastError());
    WIN_TRY(hipMemcpy(out_i, o.out_i, (size_t)fns.n * n * 8, hipMemcpyDeviceToHost));
    WIN_TRY(hipMemcpy(out_d, o.out_d, (size_t)fns.n * n * 8, hipMemcpyDeviceToHost));
    WIN_TRY(hipMemcpy(out_null, o.out_null, (size_t)fns.n * n, hipMemcpyDeviceToHost));
    return 0;
}

/* the full window pipeline. Returns rows produced (= rows passing q), <0 on
 * error. Outputs fn-major: out_i/out_d/out_null[f*n + i], rows in
 * (partition, order, arrival) order with their global ids in out_rowids.
 * frame_mode is a BkFrameMode (bk_common.h; win_frame_bounds defines each).
 * All frame modes support SUM/COUNT/COUNT(*)/AVG/MIN/MAX and
 * FIRST/LAST/NTH_VALUE (RowFrame/RangeFrameWindowProcessor,
 * window_node.cpp:49-58). */
extern "C" int64_t bkgpu_window_multi(BkgTable* t, const BkQuerySpec* q,
                                const int32_t* part_cols, int32_t n_part,
                                const BkOrderSpec* order, int norder,
                                const BkWindowFn* fns, int nfns,
                                int32_t frame_mode, int64_t f_pre, int64_t f_fol,
                                int64_t row_begin, int64_t row_end,
                                int64_t* out_rowids, int64_t* out_i,
                                double* out_d, uint8_t* out_null) {
    if (win_check_args(t, part_cols, n_part, order, norder, fns, nfns,
                       frame_mode) < 0)
        return -1;
    WinCompareCols w{};
    w.n_part = n_part;
    for (int k = 0; k < n_part; k++) w.part[k] = part_cols[k];
    w.n_ord = norder;
    for (int k = 0; k < norder; k++) w.ord[k] = order[k].col;
    PoolBufs bufs;
    WinStream s{};
    int64_t n = win_sort(bufs, t, q, w, order, row_begin, row_end, out_rowids, s);
    if (n <= 0) return n;

    WinFns wf{fns, nullptr, nfns};
    WIN_TRY(bufs.get(&wf.d, sizeof(BkWindowFn) * (size_t)nfns));
    WIN_TRY(hipMemcpy(wf.d, fns, sizeof(BkWindowFn) * (size_t)nfns,
                      hipMemcpyHostToDevice));
    DevCols dc = table_cols(t);
    WinFrame fm{frame_mode, norder >= 1 ? order[0].col : -1,
                norder >= 1 ? order[0].is_null_first : 1, f_pre, f_fol};
    WinFrameIn in{};
    if (win_structure(bufs, dc, w, wf, s) < 0) return -1;
    if (frame_mode != BK_FRAME_NONE &&
        (win_frame_prefixes(bufs, t, dc, s, wf, in) < 0 ||
         win_sparse_table(bufs, dc, s, fm, wf, in) < 0))
        return -1;
    if (win_emit_download(bufs, dc, s, fm, in, wf, out_i, out_d, out_null) < 0)
        return -1;
    return n;
}

/* single-partition-column compatibility entry (the round-1 surface) */
extern "C" int64_t bkgpu_window(BkgTable* t, const BkQuerySpec* q,
                                int32_t part_col,
                                const BkOrderSpec* order, int norder,
                                const BkWindowFn* fns, int nfns,
                                int32_t frame_mode, int64_t f_pre,
                                int64_t f_fol, int64_t row_begin,
                                int64_t row_end, int64_t* out_rowids,
                                int64_t* out_i, double* out_d,
                                uint8_t* out_null) {
    int32_t pc[1] = {part_col};
    return bkgpu_window_multi(t, q, pc, part_col >= 0 ? 1 : 0, order,
                              norder, fns, nfns, frame_mode, f_pre, f_fol,
                              row_begin, row_end, out_rowids, out_i, out_d,
                              out_null);
}

#undef WIN_TRY
#undef WIN_LAUNCH

# WindowNode (NON-FRAME mode, window_node.cpp:39-41 + window_fn_call.cpp):
# oracle vs numpy brute force (CPU) and GPU vs oracle (parity).
import numpy as np
import pytest

TYPE_INT64, TYPE_DOUBLE, TYPE_STRING = 6, 12, 13
D_UNI, D_SKEW, D_DICT, D_SUM16 = 0, 1, 2, 3
W = {"count_star": 0, "count": 1, "sum": 2, "avg": 3, "min": 4, "max": 5,
     "row_number": 10, "rank": 11, "dense_rank": 12, "percent_rank": 13,
     "first_value": 14, "last_value": 15, "nth_value": 16, "lead": 17,
     "lag": 18, "cume_dist": 19, "ntile": 20}
SEED = 77


def gen(orc, specs, n, seed=SEED):
    import ctypes as C
    from oracle.bindings import BkColSpec
    arr = (BkColSpec * len(specs))()
    for i, s in enumerate(specs):
        (arr[i].col_type, arr[i].dist, arr[i].p0, arr[i].p1,
         arr[i].null_frac_x1e6) = s
    cols, valids = orc.generate_table(list(arr), n, seed)
    return cols, valids, [s[0] for s in specs]


@pytest.fixture(scope="module")
def orc():
    from oracle import Oracle
    return Oracle()


@pytest.fixture(scope="module")
def eng():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    from baikaldb_amd import GpuEngine
    return GpuEngine()


def brute_window(cols, valids, part_col, order, fns):
    """numpy/python reference independent of oracle code paths."""
    n = len(cols[0])

    def null(c, r):
        return valids[c] is not None and valids[c][r] == 0

    def keyf(r):
        ks = []
        if part_col >= 0:
            ks.append((0 if null(part_col, r) else 1,
                       None if null(part_col, r) else cols[part_col][r]))
        for col, asc, nf in order:
            isn = null(col, r)
            v = None if isn else cols[col][r]
            # null_first under asc: nulls smallest; invert value for desc
            nk = (0 if nf else 2) if isn else 1
            ks.append((nk, (v if asc else (-v if v is not None else None))
                       if not isn else 0))
        ks.append(r)
        return tuple(ks)

    idx = sorted(range(n), key=keyf)
    out = {f: [None] * n for f in range(len(fns))}
    # partitions
    def peq(a, b):
        if part_col < 0:
            return True
        na, nb = null(part_col, a), null(part_col, b)
        if na != nb:
            return False
        return na or cols[part_col][a] == cols[part_col][b]

    def oeq(a, b):
        for col, _, _ in order:
            na, nb = null(col, a), null(col, b)
            if na != nb:
                return False
            if not na and cols[col][a] != cols[col][b]:
                return False
        return True

    ps = 0
    while ps < n:
        pe = ps + 1
        while pe < n and peq(idx[pe], idx[pe - 1]):
            pe += 1
        rows = [idx[j] for j in range(ps, pe)]
        pn = len(rows)
        for f, (name, col, *rest) in enumerate(fns):
            param = rest[0] if rest else 0
            if name == "count_star":
                vals = [pn] * pn
            elif name == "count":
                c = sum(0 if null(col, r) else 1 for r in rows)
                vals = [c] * pn
            elif name in ("sum", "avg", "min", "max"):
                vv = [cols[col][r] for r in rows if not null(col, r)]
                if not vv:
                    vals = [None] * pn
                elif name == "sum":
                    vals = [np.sum(np.array(vv))] * pn
                elif name == "avg":
                    vals = [float(np.mean(np.array(vv, dtype=np.float64)))] * pn
                elif name == "min":
                    vals = [min(vv)] * pn
                else:
                    vals = [max(vv)] * pn
            elif name == "row_number":
                vals = list(range(1, pn + 1))
            elif name in ("rank", "dense_rank", "percent_rank"):
                vals = []
                rank, dense = 1, 1
                for j in range(pn):
                    if j > 0 and not oeq(rows[j], rows[j - 1]):
                        rank = j + 1
                        dense += 1
                    if name == "rank":
                        vals.append(rank)
                    elif name == "dense_rank":
                        vals.append(dense)
                    else:
                        vals.append((rank - 1) / (pn - 1) if pn > 1 else 0.0)
            elif name == "first_value":
                r0 = rows[0]
                vals = [None if null(col, r0) else cols[col][r0]] * pn
            elif name == "last_value":
                r0 = rows[-1]
                vals = [None if null(col, r0) else cols[col][r0]] * pn
            elif name == "nth_value":
                j = param - 1
                if 0 <= j < pn:
                    r0 = rows[j]
                    vals = [None if null(col, r0) else cols[col][r0]] * pn
                else:
                    vals = [None] * pn
            elif name == "cume_dist":
                vals = []
                for j in range(pn):
                    le = j + 1
                    while le < pn and oeq(rows[le], rows[j]):
                        le += 1
                    vals.append(le / pn)
            elif name == "ntile":
                k = param if param > 0 else 1
                quot, rem = pn // k, pn % k
                fat = rem * (quot + 1)
                vals = [(j // (quot + 1) + 1) if j < fat
                        else rem + ((j - fat) // quot if quot else 0) + 1
                        for j in range(pn)]
            elif name in ("lead", "lag"):
                off = param if param > 0 else 1
                vals = []
                for j in range(pn):
                    jj = j + off if name == "lead" else j - off
                    if 0 <= jj < pn and not null(col, rows[jj]):
                        vals.append(cols[col][rows[jj]])
                    else:
                        vals.append(None)
            else:
                raise ValueError(name)
            for j in range(pn):
                out[f][ps + j] = vals[j]
        ps = pe
    return idx, out


FNS = [("count_star", -1), ("count", 2), ("sum", 2), ("avg", 2),
       ("min", 2), ("max", 2), ("row_number", -1), ("rank", -1)]
FNS2 = [("dense_rank", -1), ("percent_rank", -1), ("first_value", 2),
        ("last_value", 2), ("nth_value", 2, 3), ("lead", 2, 1), ("lag", 2, 2)]
FNS3 = [("cume_dist", -1, 0), ("ntile", -1, 4), ("ntile", -1, 7),
        ("rank", -1), ("row_number", -1)]


def check_against_brute(res, col_types, fns, idx, brute):
    assert res["n"] == len(idx)
    assert np.array_equal(res["rowids"], np.array(idx))
    for f, fdesc in enumerate(fns):
        name, col = fdesc[0], fdesc[1]
        is_double = (name in ("avg", "percent_rank", "cume_dist") or
                     (col >= 0 and col_types[col] == TYPE_DOUBLE))
        for i in range(res["n"]):
            b = brute[f][i]
            if b is None:
                assert res["out_null"][f][i] == 1, (name, i)
            else:
                assert res["out_null"][f][i] == 0, (name, i, b)
                if is_double:
                    got = res["out_d"][f][i]
                    assert abs(got - b) <= 1e-9 * (abs(b) + 1), (name, i, got, b)
                else:
                    assert res["out_i"][f][i] == b, (name, i)


def oracle_window(orc, cols, valids, col_types, fns, part_col, order):
    ofns = [(W[f[0]], f[1], f[2] if len(f) > 2 else 0) for f in fns]
    return orc.window(cols, valids, col_types, ofns, part_col=part_col,
                      order=order)


def test_oracle_window_vs_brute(orc):
    specs = [(TYPE_INT64, D_UNI, 0, 12, 0),          # partition
             (TYPE_INT64, D_UNI, 0, 40, 100_000),    # order key, 10% null
             (TYPE_INT64, D_UNI, -500, 500, 200_000)]  # value, 20% null
    cols, valids, types = gen(orc, specs, 4000)
    order = [(1, 1, 1)]
    for fns in (FNS, FNS2, FNS3):
        res = oracle_window(orc, cols, valids, types, fns, 0, order)
        idx, brute = brute_window(cols, valids, 0, order, fns)
        check_against_brute(res, types, fns, idx, brute)


def test_oracle_window_no_partition_no_order(orc):
    specs = [(TYPE_INT64, D_UNI, 0, 100, 0)]
    cols, valids, types = gen(orc, specs, 500)
    fns = [("row_number", -1), ("rank", -1), ("count_star", -1)]
    res = oracle_window(orc, cols, valids, types, fns, -1, [])
    assert res["n"] == 500
    assert np.array_equal(res["out_i"][0], np.arange(1, 501))  # row_number
    assert np.all(res["out_i"][1] == 1)                        # rank: no order
    assert np.all(res["out_i"][2] == 500)


@pytest.mark.gpu
@pytest.mark.parametrize("fns", [FNS, FNS2, FNS3])
def test_gpu_window_parity(eng, orc, fns):
    specs = [(TYPE_INT64, D_UNI, 0, 300, 50_000),      # partition, nullable
             (TYPE_INT64, D_UNI, 0, 25, 100_000),      # order
             (TYPE_DOUBLE, D_SUM16, 0, 0, 150_000),    # double value
             (TYPE_INT64, D_UNI, 0, 1 << 31, 0)]
    # swap value col to the double col for a double-typed run
    fns = [tuple([f[0], 2 if f[1] == 2 else f[1]] + list(f[2:])) for f in fns]
    n = 200_000
    from baikaldb_amd import QueryPlan
    t = eng.create_table(specs, n)
    try:
        eng.generate(t, SEED)
        plan = QueryPlan(t.col_types, conjuncts=[(3, "<", 1 << 30)])
        got = eng.window(t, fns, part_col=0, order=[(1, 1, 1)], plan=plan)
    finally:
        t.free()
    cols, valids, types = gen(orc, specs, n)
    from oracle.bindings import make_query
    q = make_query([(3, 4, TYPE_INT64, 1 << 30)], (), ((0, -1),), types)
    q.n_aggs = 0
    exp = orc.window(cols, valids, types,
                     [(W[f[0]], f[1], f[2] if len(f) > 2 else 0) for f in fns],
                     part_col=0, order=[(1, 1, 1)], q=q)
    assert got["n"] == exp["n"]
    assert np.array_equal(got["rowids"], exp["rowids"])
    assert np.array_equal(got["out_null"], exp["out_null"])
    assert np.array_equal(got["out_i"], exp["out_i"])
    mask = exp["out_null"] == 0
    d = np.abs(got["out_d"] - exp["out_d"])
    tol = 1e-10 * (np.abs(exp["out_d"]) + 100)
    assert np.all(d[mask] <= tol[mask])


@pytest.mark.gpu
def test_gpu_window_desc_order_and_big_partitions(eng, orc):
    specs = [(TYPE_INT64, D_UNI, 0, 3, 0),             # 3 huge partitions
             (TYPE_INT64, D_UNI, 0, 1 << 40, 0),
             (TYPE_INT64, D_UNI, 0, 1000, 0)]
    n = 300_000
    fns = [("row_number", -1), ("rank", -1), ("sum", 2), ("lag", 2, 3)]
    t = eng.create_table(specs, n)
    try:
        eng.generate(t, SEED + 1)
        got = eng.window(t, fns, part_col=0, order=[(1, 0, 0)])  # desc
    finally:
        t.free()
    cols, valids, types = gen(orc, specs, n, SEED + 1)
    exp = orc.window(cols, valids, types,
                     [(W[f[0]], f[1], f[2] if len(f) > 2 else 0) for f in fns],
                     part_col=0, order=[(1, 0, 0)])
    assert got["n"] == exp["n"] == n
    assert np.array_equal(got["rowids"], exp["rowids"])
    assert np.array_equal(got["out_i"], exp["out_i"])
    assert np.array_equal(got["out_null"], exp["out_null"])


@pytest.mark.gpu
@pytest.mark.parametrize("case_seed", range(3))
def test_gpu_window_fuzz(eng, orc, case_seed):
    """Randomized schemas x window specs: GPU vs oracle (oracle itself is
    pinned against the numpy brute force above)."""
    import random
    rng = random.Random(4200 + case_seed)
    for sub in range(4):
        ncols = rng.randint(2, 5)
        specs = []
        for _ in range(ncols):
            tcol = rng.choice([TYPE_INT64, TYPE_INT64, TYPE_DOUBLE])
            nf = rng.choice([0, 0, 200_000])
            if tcol == TYPE_INT64:
                specs.append((tcol, D_UNI, 0,
                              rng.choice([5, 50, 1 << 20, 1 << 40]), nf))
            else:
                specs.append((tcol, D_SUM16, 0, 0, nf))
        part = rng.choice([-1] + list(range(ncols)))
        n_ord = rng.randint(0, min(2, ncols))
        order = [(c, rng.randint(0, 1), rng.randint(0, 1))
                 for c in rng.sample(range(ncols), n_ord)]
        pool = list(W.keys())
        fns = []
        for _ in range(rng.randint(1, 6)):
            name = rng.choice(pool)
            needs_col = name not in ("count_star", "row_number", "rank",
                                     "dense_rank", "percent_rank",
                                     "cume_dist", "ntile")
            col = rng.randrange(ncols) if needs_col else -1
            param = rng.randint(1, 5) if name in ("nth_value", "lead",
                                                  "lag", "ntile") else 0
            fns.append((name, col, param))
        n = rng.choice([3000, 20_000])
        seed = rng.randrange(1 << 40)
        # random frame mode; frames restrict to the fns they define
        frame = rng.choice([None, None, (rng.randint(0, 4), rng.randint(0, 4)),
                            (-1, 0), "range_upc", "range_crf"])
        if frame is not None:
            fns = [f for f in fns
                   if f[0] in ("count_star", "count", "sum", "avg", "min",
                               "max", "first_value", "last_value",
                               "nth_value", "row_number", "rank",
                               "dense_rank", "lead", "lag")]
            if not fns:
                fns = [("count_star", -1, 0)]
        t = eng.create_table(specs, n)
        try:
            eng.generate(t, seed)
            got = eng.window(t, fns, part_col=part, order=order, frame=frame)
        finally:
            t.free()
        cols, valids, types = gen(orc, specs, n, seed)
        exp = orc.window(cols, valids, types,
                         [(W[f[0]], f[1], f[2]) for f in fns],
                         part_col=part, order=order, frame=frame)
        ctx = f"fuzz {case_seed}/{sub} part={part} order={order} fns={fns}"
        assert got["n"] == exp["n"], ctx
        assert np.array_equal(got["rowids"], exp["rowids"]), ctx
        assert np.array_equal(got["out_null"], exp["out_null"]), ctx
        assert np.array_equal(got["out_i"], exp["out_i"]), ctx
        mask = exp["out_null"] == 0
        d = np.abs(got["out_d"] - exp["out_d"])
        tol = 1e-10 * (np.abs(exp["out_d"]) + 100)
        assert np.all(d[mask] <= tol[mask]), ctx


def brute_frame(cols, valids, part_col, order, fns, pre, fol):
    """ROWS-frame brute force for SUM/COUNT/AVG/first/last/nth."""
    idx, _ = brute_window(cols, valids, part_col, order,
                          [("row_number", -1)])
    n = len(idx)

    def null(c, r):
        return valids[c] is not None and valids[c][r] == 0

    def peq(a, b):
        if part_col < 0:
            return True
        na, nb = null(part_col, a), null(part_col, b)
        return na == nb and (na or cols[part_col][a] == cols[part_col][b])

    out = {f: [None] * n for f in range(len(fns))}
    ps = 0
    while ps < n:
        pe = ps + 1
        while pe < n and peq(idx[pe], idx[pe - 1]):
            pe += 1
        for j in range(ps, pe):
            fl = ps if pre < 0 else max(ps, j - pre)
            fr = pe - 1 if fol < 0 else min(pe - 1, j + fol)
            frame_rows = [idx[k] for k in range(fl, fr + 1)]
            for f, (name, col, *rest) in enumerate(fns):
                param = rest[0] if rest else 0
                if name == "count_star":
                    out[f][j] = len(frame_rows)
                elif name == "count":
                    out[f][j] = sum(0 if null(col, r) else 1
                                    for r in frame_rows)
                elif name in ("sum", "avg"):
                    vv = [cols[col][r] for r in frame_rows if not null(col, r)]
                    if not vv:
                        out[f][j] = None
                    elif name == "sum":
                        out[f][j] = np.sum(np.array(vv))
                    else:
                        out[f][j] = float(np.mean(np.array(vv,
                                                           dtype=np.float64)))
                elif name in ("min", "max"):
                    vv = [cols[col][r] for r in frame_rows if not null(col, r)]
                    out[f][j] = (min(vv) if name == "min" else max(vv)) \
                        if vv else None
                elif name == "first_value":
                    r = frame_rows[0]
                    out[f][j] = None if null(col, r) else cols[col][r]
                elif name == "last_value":
                    r = frame_rows[-1]
                    out[f][j] = None if null(col, r) else cols[col][r]
                elif name == "nth_value":
                    k = param - 1
                    if 0 <= k < len(frame_rows):
                        r = frame_rows[k]
                        out[f][j] = None if null(col, r) else cols[col][r]
                    else:
                        out[f][j] = None
        ps = pe
    return idx, out


FRAME_FNS = [("count_star", -1), ("count", 2), ("sum", 2), ("avg", 2),
             ("first_value", 2), ("last_value", 2), ("nth_value", 2, 2),
             ("min", 2)]


@pytest.mark.parametrize("frame", [(-1, 0), (3, 0), (0, 3), (2, 2)])
def test_oracle_rows_frame_vs_brute(orc, frame):
    specs = [(TYPE_INT64, D_UNI, 0, 10, 0),
             (TYPE_INT64, D_UNI, 0, 30, 100_000),
             (TYPE_INT64, D_UNI, -100, 100, 200_000)]
    cols, valids, types = gen(orc, specs, 2500)
    order = [(1, 1, 1)]
    res = orc.window(cols, valids, types,
                     [(W[f[0]], f[1], f[2] if len(f) > 2 else 0)
                      for f in FRAME_FNS],
                     part_col=0, order=order, frame=frame)
    idx, brute = brute_frame(cols, valids, 0, order, FRAME_FNS, *frame)
    check_against_brute(res, types, FRAME_FNS, idx, brute)


@pytest.mark.gpu
@pytest.mark.parametrize("frame", [(-1, 0), (5, 0), (1, 4)])
def test_gpu_rows_frame_parity(eng, orc, frame):
    specs = [(TYPE_INT64, D_UNI, 0, 200, 50_000),
             (TYPE_INT64, D_UNI, 0, 40, 0),
             (TYPE_DOUBLE, D_SUM16, 0, 0, 150_000),
             (TYPE_INT64, D_UNI, -500, 500, 100_000)]
    fns = [("count_star", -1), ("sum", 3), ("min", 3), ("max", 2),
           ("count", 3), ("first_value", 3), ("last_value", 2),
           ("nth_value", 3, 3)]
    n = 150_000
    t = eng.create_table(specs, n)
    try:
        eng.generate(t, SEED + 5)
        got = eng.window(t, fns, part_col=0, order=[(1, 1, 1)], frame=frame)
    finally:
        t.free()
    cols, valids, types = gen(orc, specs, n, SEED + 5)
    exp = orc.window(cols, valids, types,
                     [(W[f[0]], f[1], f[2] if len(f) > 2 else 0) for f in fns],
                     part_col=0, order=[(1, 1, 1)], frame=frame)
    assert got["n"] == exp["n"]
    assert np.array_equal(got["rowids"], exp["rowids"])
    assert np.array_equal(got["out_null"], exp["out_null"])
    assert np.array_equal(got["out_i"], exp["out_i"])
    mask = exp["out_null"] == 0
    d = np.abs(got["out_d"] - exp["out_d"])
    tol = 1e-9 * (np.abs(exp["out_d"]) + 100)
    assert np.all(d[mask] <= tol[mask])


def brute_range_frame(cols, valids, part_col, order, fns, mode):
    """RANGE frames: upc = [ps, peer_end), crf = [peer_head, pe)."""
    idx, _ = brute_window(cols, valids, part_col, order, [("row_number", -1)])
    n = len(idx)

    def null(c, r):
        return valids[c] is not None and valids[c][r] == 0

    def peq(a, b):
        if part_col < 0:
            return True
        na, nb = null(part_col, a), null(part_col, b)
        return na == nb and (na or cols[part_col][a] == cols[part_col][b])

    def oeq(a, b):
        for col, _, _ in order:
            na, nb = null(col, a), null(col, b)
            if na != nb:
                return False
            if not na and cols[col][a] != cols[col][b]:
                return False
        return True

    out = {f: [None] * n for f in range(len(fns))}
    ps = 0
    while ps < n:
        pe = ps + 1
        while pe < n and peq(idx[pe], idx[pe - 1]):
            pe += 1
        for j in range(ps, pe):
            lo, hi = j, j
            while lo > ps and oeq(idx[lo - 1], idx[j]):
                lo -= 1
            while hi + 1 < pe and oeq(idx[hi + 1], idx[j]):
                hi += 1
            fl, fr = (ps, hi) if mode == "range_upc" else (lo, pe - 1)
            frame_rows = [idx[k] for k in range(fl, fr + 1)]
            for f, (name, col, *rest) in enumerate(fns):
                if name == "count_star":
                    out[f][j] = len(frame_rows)
                elif name == "sum":
                    vv = [cols[col][r] for r in frame_rows if not null(col, r)]
                    out[f][j] = np.sum(np.array(vv)) if vv else None
        ps = pe
    return idx, out


@pytest.mark.parametrize("mode", ["range_upc", "range_crf"])
def test_oracle_range_frame_vs_brute(orc, mode):
    specs = [(TYPE_INT64, D_UNI, 0, 8, 0),
             (TYPE_INT64, D_UNI, 0, 12, 100_000),   # coarse: many ties
             (TYPE_INT64, D_UNI, -50, 50, 0)]
    cols, valids, types = gen(orc, specs, 2000)
    order = [(1, 1, 1)]
    fns = [("count_star", -1), ("sum", 2)]
    res = orc.window(cols, valids, types,
                     [(W[f[0]], f[1], 0) for f in fns],
                     part_col=0, order=order, frame=mode)
    idx, brute = brute_range_frame(cols, valids, 0, order, fns, mode)
    check_against_brute(res, types, fns, idx, brute)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["range_upc", "range_crf"])
def test_gpu_range_frame_parity(eng, orc, mode):
    specs = [(TYPE_INT64, D_UNI, 0, 100, 0),
             (TYPE_INT64, D_UNI, 0, 15, 50_000),
             (TYPE_INT64, D_UNI, -500, 500, 100_000)]
    fns = [("count_star", -1), ("sum", 2), ("avg", 2), ("last_value", 2)]
    n = 120_000
    t = eng.create_table(specs, n)
    try:
        eng.generate(t, SEED + 9)
        got = eng.window(t, fns, part_col=0, order=[(1, 1, 1)], frame=mode)
    finally:
        t.free()
    cols, valids, types = gen(orc, specs, n, SEED + 9)
    exp = orc.window(cols, valids, types,
                     [(W[f[0]], f[1], 0) for f in fns],
                     part_col=0, order=[(1, 1, 1)], frame=mode)
    assert got["n"] == exp["n"]
    assert np.array_equal(got["rowids"], exp["rowids"])
    assert np.array_equal(got["out_null"], exp["out_null"])
    assert np.array_equal(got["out_i"], exp["out_i"])
    mask = exp["out_null"] == 0
    d = np.abs(got["out_d"] - exp["out_d"])
    tol = 1e-9 * (np.abs(exp["out_d"]) + 100)
    assert np.all(d[mask] <= tol[mask])


def test_oracle_lead_lag_default(orc):
    """LEAD/LAG with a literal default (window_fn_call.cpp:144-150)."""
    specs = [(TYPE_INT64, D_UNI, 0, 5, 0),
             (TYPE_INT64, D_UNI, 0, 100, 0)]
    cols, valids, types = gen(orc, specs, 400)
    fns = [(W["lag"], 1, 2, -777), (W["lead"], 1, 1, 999)]
    res = orc.window(cols, valids, types, fns, part_col=0, order=[(1, 1, 1)])
    idx, brute = brute_window(cols, valids, 0, [(1, 1, 1)],
                              [("lag", 1, 2), ("lead", 1, 1)])
    for f, dflt in ((0, -777), (1, 999)):
        for i in range(res["n"]):
            b = brute[f][i]
            assert res["out_null"][f][i] == 0
            assert res["out_i"][f][i] == (dflt if b is None else b), (f, i)


@pytest.mark.gpu
def test_gpu_lead_lag_default(eng, orc):
    specs = [(TYPE_INT64, D_UNI, 0, 50, 0),
             (TYPE_INT64, D_UNI, 0, 1 << 20, 0),
             (TYPE_DOUBLE, D_SUM16, 0, 0, 100_000)]
    fns = [("lag", 1, 1, -5), ("lead", 2, 3, 2.5), ("lead", 1, 2)]
    n = 80_000
    t = eng.create_table(specs, n)
    try:
        eng.generate(t, SEED + 3)
        got = eng.window(t, fns, part_col=0, order=[(1, 1, 1)])
    finally:
        t.free()
    cols, valids, types = gen(orc, specs, n, SEED + 3)
    exp = orc.window(cols, valids, types,
                     [(W[f[0]], f[1], f[2], f[3] if len(f) > 3 else None)
                      for f in fns],
                     part_col=0, order=[(1, 1, 1)])
    assert np.array_equal(got["out_null"], exp["out_null"])
    assert np.array_equal(got["out_i"], exp["out_i"])
    mask = exp["out_null"] == 0
    assert np.allclose(got["out_d"][mask], exp["out_d"][mask], rtol=1e-12)


def brute_range_val(cols, valids, part_col, order, fns, pre, fol):
    """RANGE value-offset frames, single ASC int key."""
    idx, _ = brute_window(cols, valids, part_col, order, [("row_number", -1)])
    n = len(idx)
    oc = order[0][0]

    def null(c, r):
        return valids[c] is not None and valids[c][r] == 0

    def peq(a, b):
        if part_col < 0:
            return True
        na, nb = null(part_col, a), null(part_col, b)
        return na == nb and (na or cols[part_col][a] == cols[part_col][b])

    out = {f: [None] * n for f in range(len(fns))}
    ps = 0
    while ps < n:
        pe = ps + 1
        while pe < n and peq(idx[pe], idx[pe - 1]):
            pe += 1
        for j in range(ps, pe):
            if null(oc, idx[j]):
                fl = j
                while fl > ps and null(oc, idx[fl - 1]):
                    fl -= 1
                fr = j
                while fr + 1 < pe and null(oc, idx[fr + 1]):
                    fr += 1
            else:
                v = cols[oc][idx[j]]
                fl = fr = j
                while fl > ps and not null(oc, idx[fl - 1]) and \
                        (pre < 0 or cols[oc][idx[fl - 1]] >= v - pre):
                    fl -= 1
                while fr + 1 < pe and not null(oc, idx[fr + 1]) and \
                        (fol < 0 or cols[oc][idx[fr + 1]] <= v + fol):
                    fr += 1
            frame_rows = [idx[k] for k in range(fl, fr + 1)]
            for f, (name, col, *rest) in enumerate(fns):
                if name == "count_star":
                    out[f][j] = len(frame_rows)
                elif name == "sum":
                    vv = [cols[col][r] for r in frame_rows if not null(col, r)]
                    out[f][j] = np.sum(np.array(vv)) if vv else None
                elif name == "min":
                    vv = [cols[col][r] for r in frame_rows if not null(col, r)]
                    out[f][j] = min(vv) if vv else None
                elif name == "first_value":
                    r0 = frame_rows[0]
                    out[f][j] = None if null(col, r0) else cols[col][r0]
                elif name == "last_value":
                    r0 = frame_rows[-1]
                    out[f][j] = None if null(col, r0) else cols[col][r0]
        ps = pe
    return idx, out


@pytest.mark.parametrize("vframe", [(10, 10), (0, 25), (-1, 5)])
def test_oracle_range_val_vs_brute(orc, vframe):
    specs = [(TYPE_INT64, D_UNI, 0, 6, 0),
             (TYPE_INT64, D_UNI, 0, 200, 150_000),
             (TYPE_INT64, D_UNI, -40, 40, 0)]
    cols, valids, types = gen(orc, specs, 2000)
    order = [(1, 1, 1)]
    fns = [("count_star", -1), ("sum", 2), ("min", 2), ("last_value", 2),
           ("first_value", 2)]
    res = orc.window(cols, valids, types, [(W[f[0]], f[1], 0) for f in fns],
                     part_col=0, order=order,
                     frame=("range_val", vframe[0], vframe[1]))
    idx, brute = brute_range_val(cols, valids, 0, order, fns, *vframe)
    check_against_brute(res, types, fns, idx, brute)


@pytest.mark.gpu
@pytest.mark.parametrize("vframe", [(100, 100), (-1, 50)])
def test_gpu_range_val_parity(eng, orc, vframe):
    specs = [(TYPE_INT64, D_UNI, 0, 60, 0),
             (TYPE_INT64, D_UNI, 0, 5000, 120_000),
             (TYPE_INT64, D_UNI, -900, 900, 80_000)]
    fns = [("count_star", -1), ("sum", 2), ("avg", 2), ("min", 2),
           ("max", 2), ("last_value", 2)]
    n = 120_000
    t = eng.create_table(specs, n)
    try:
        eng.generate(t, SEED + 11)
        got = eng.window(t, fns, part_col=0, order=[(1, 1, 1)],
                         frame=("range_val", vframe[0], vframe[1]))
    finally:
        t.free()
    cols, valids, types = gen(orc, specs, n, SEED + 11)
    exp = orc.window(cols, valids, types, [(W[f[0]], f[1], 0) for f in fns],
                     part_col=0, order=[(1, 1, 1)],
                     frame=("range_val", vframe[0], vframe[1]))
    assert got["n"] == exp["n"]
    assert np.array_equal(got["rowids"], exp["rowids"])
    assert np.array_equal(got["out_null"], exp["out_null"])
    assert np.array_equal(got["out_i"], exp["out_i"])
    mask = exp["out_null"] == 0
    d = np.abs(got["out_d"] - exp["out_d"])
    tol = 1e-9 * (np.abs(exp["out_d"]) + 100)
    assert np.all(d[mask] <= tol[mask])


_TABLES = {}


def gpu_vs_oracle(eng, orc, specs, n, seed, fns, part_col, order, frame=None):
    """One engine window call and the oracle's answer on the same seeded
    table (generated once per (specs, n, seed)); asserts the frame tests'
    comparison block and returns the oracle result for case-shape checks."""
    t = eng.create_table(specs, n)
    try:
        eng.generate(t, seed)
        got = eng.window(t, fns, part_col=part_col, order=order, frame=frame)
    finally:
        t.free()
    key = (tuple(specs), n, seed)
    if key not in _TABLES:
        _TABLES[key] = gen(orc, specs, n, seed)
    cols, valids, types = _TABLES[key]
    exp = orc.window(cols, valids, types,
                     [(W[f[0]], f[1], f[2] if len(f) > 2 else 0,
                       f[3] if len(f) > 3 else None) for f in fns],
                     part_col=part_col, order=order, frame=frame)
    assert got["n"] == exp["n"]
    assert np.array_equal(got["rowids"], exp["rowids"])
    assert np.array_equal(got["out_null"], exp["out_null"])
    assert np.array_equal(got["out_i"], exp["out_i"])
    mask = exp["out_null"] == 0
    d = np.abs(got["out_d"] - exp["out_d"])
    tol = 1e-9 * (np.abs(exp["out_d"]) + 100)
    assert np.all(d[mask] <= tol[mask])
    return exp


NULLY_SPECS = [(TYPE_INT64, D_UNI, 0, 8, 0),
               (TYPE_INT64, D_UNI, 0, 50, 100_000),
               (TYPE_INT64, D_UNI, -500, 500, 850_000),
               (TYPE_DOUBLE, D_SUM16, 0, 0, 850_000),
               (TYPE_STRING, D_DICT, 64, 0, 850_000)]


@pytest.mark.gpu
@pytest.mark.parametrize("order", [[(1, 1, 1)], [(1, 1, 0)]])
@pytest.mark.parametrize("frame", [(1, 1), (3, 4)])
def test_gpu_rows_frame_mostly_null_values(eng, orc, frame, order):
    """85%-NULL value columns: frames with no value (NULL result) next to
    frames with some, for every aggregate family incl. STRING MIN/MAX. The
    (3, 4) frame is 8 rows long: the sparse-table level on an exact power of
    two."""
    fns = [("sum", 2), ("min", 2), ("max", 3), ("avg", 3), ("min", 4),
           ("max", 4), ("count", 2), ("first_value", 4)]
    exp = gpu_vs_oracle(eng, orc, NULLY_SPECS, 4000, 101, fns, 0, order, frame)
    for f in range(6):    # SUM/MIN/MAX/AVG: NULL and non-NULL results both occur
        nulls = int(exp["out_null"][f].sum())
        assert 0 < nulls < exp["n"], (fns[f], nulls)
    assert not exp["out_null"][6].any()   # COUNT is never NULL


EDGE64_SPECS = [(TYPE_INT64, D_UNI, 0, 4, 0),
                (TYPE_INT64, D_UNI, 0, 1 << 40, 0),
                (TYPE_INT64, D_UNI, 0, 1 << 40, 100_000),
                (TYPE_DOUBLE, D_SUM16, 0, 0, 100_000)]


@pytest.mark.gpu
@pytest.mark.parametrize("frame,longest", [((31, 32), 64), ((32, 32), 65)])
def test_gpu_rows_frame_direct_sum_boundary(eng, orc, frame, longest):
    """Either side of the 64-row rule of the frame SUM/AVG evaluator: full
    64-row frames are summed in frame order, 65-row frames take the prefix
    difference; partition edges give shorter frames in both cases."""
    fns = [("avg", 2), ("sum", 3), ("count_star", -1)]
    exp = gpu_vs_oracle(eng, orc, EDGE64_SPECS, 3000, 102, fns, 0, [(1, 1, 1)],
                        frame)
    rows = exp["out_i"][2]
    assert rows.max() == longest
    assert rows.min() < longest


@pytest.mark.gpu
@pytest.mark.parametrize("null_first", [1, 0])
def test_gpu_range_val_null_keys_either_end(eng, orc, null_first):
    """RANGE by value with the NULL order keys sorted first or last: the
    non-null span the binary searches run over is clipped at either end."""
    specs = [(TYPE_INT64, D_UNI, 0, 6, 0),
             (TYPE_INT64, D_UNI, 0, 300, 200_000),
             (TYPE_INT64, D_UNI, -40, 40, 300_000)]
    fns = [("count_star", -1), ("min", 2), ("sum", 2), ("avg", 2)]
    exp = gpu_vs_oracle(eng, orc, specs, 3000, 103, fns, 0,
                        [(1, 1, null_first)], ("range_val", 7, 0))
    rows = exp["out_i"][0]
    assert rows.min() == 1 and rows.max() > 64   # both AVG sum routes


@pytest.mark.gpu
def test_gpu_window_eight_fns_all_families(eng, orc):
    """BK_MAX_WINFNS fns in one non-frame call, one per family, LEAD with a
    float default on a DOUBLE column. Ordered by the nullable c2, so each
    partition's NULL keys form one large peer group."""
    fns = [("count_star", -1), ("sum", 3), ("min", 2), ("dense_rank", -1),
           ("cume_dist", -1), ("ntile", -1, 7), ("nth_value", 2, 3),
           ("lead", 3, 2, 0.5)]
    exp = gpu_vs_oracle(eng, orc, EDGE64_SPECS, 3000, 102, fns, 0,
                        [(2, 1, 1), (0, 1, 1)])
    assert exp["out_i"][3].max() < exp["out_i"][0].max()   # peers not singletons


@pytest.mark.gpu
def test_gpu_window_empty_selection(eng, orc):
    """WHERE eliminates every row: window returns 0 rows cleanly."""
    from baikaldb_amd import QueryPlan
    t = eng.create_table([(TYPE_INT64, D_UNI, 0, 100, 0)], 10_000)
    try:
        eng.generate(t, 1)
        plan = QueryPlan(t.col_types, conjuncts=[(0, "<", -5)])
        got = eng.window(t, [("row_number", -1)], part_col=0, order=[],
                         plan=plan)
    finally:
        t.free()
    assert got["n"] == 0


@pytest.mark.gpu
def test_gpu_window_single_row_partitions(eng, orc):
    """Every row its own partition (distinct keys): rank fns all 1,
    aggregates identity."""
    specs = [(TYPE_INT64, D_UNI, 0, 1 << 62, 0),
             (TYPE_INT64, D_UNI, -50, 50, 0)]
    n = 5000
    t = eng.create_table(specs, n)
    try:
        eng.generate(t, 9)
        got = eng.window(t, [("row_number", -1), ("rank", -1),
                             ("percent_rank", -1), ("sum", 1), ("lag", 1, 1)],
                         part_col=0, order=[(1, 1, 1)])
    finally:
        t.free()
    assert got["n"] == n
    assert np.all(got["out_i"][0] == 1)
    assert np.all(got["out_i"][1] == 1)
    assert np.all(got["out_d"][2] == 0.0)
    assert np.all(got["out_null"][4] == 1)   # lag leaves every 1-row partition


@pytest.mark.gpu
def test_gpu_window_two_partition_cols(eng, orc):
    """PARTITION BY two columns (round-1 cap was one): a new partition
    starts when ANY partition expr changes (window_node.cpp evaluates all
    of them); engine vs oracle on identical inputs."""
    from baikaldb_amd import QueryPlan
    specs = [(TYPE_INT64, D_UNI, 0, 12, 30_000),    # p0 (nullable)
             (TYPE_STRING, D_DICT, 8, 0, 0),        # p1 dict
             (TYPE_INT64, D_UNI, 0, 40, 0),         # order
             (TYPE_DOUBLE, D_SUM16, 0, 0, 100_000)]  # value
    fns = [("row_number", -1), ("rank", -1), ("count_star", -1),
           ("sum", 3), ("max", 2), ("dense_rank", -1)]
    n = 120_000
    t = eng.create_table(specs, n)
    try:
        eng.generate(t, SEED)
        plan = QueryPlan(t.col_types, conjuncts=[(2, "<", 35)])
        got = eng.window(t, fns, part_col=[0, 1], order=[(2, 1, 1)],
                         plan=plan)
    finally:
        t.free()
    cols, valids, types = gen(orc, specs, n)
    from oracle.bindings import make_query
    q = make_query([(2, 4, TYPE_INT64, 35)], (), ((0, -1),), types)
    q.n_aggs = 0
    exp = orc.window(cols, valids, types,
                     [(W[f[0]], f[1]) for f in fns],
                     part_col=[0, 1], order=[(2, 1, 1)], q=q)
    assert got["n"] == exp["n"]
    assert np.array_equal(got["rowids"], exp["rowids"])
    assert np.array_equal(got["out_null"], exp["out_null"])
    assert np.array_equal(got["out_i"], exp["out_i"])
    mask = exp["out_null"] == 0
    d = np.abs(got["out_d"] - exp["out_d"])
    tol = 1e-10 * (np.abs(exp["out_d"]) + 100)
    assert np.all(d[mask] <= tol[mask])


@pytest.mark.gpu
def test_gpu_window_three_partition_cols(eng, orc):
    from baikaldb_amd import QueryPlan
    specs = [(TYPE_INT64, D_UNI, 0, 5, 0),
             (TYPE_INT64, D_UNI, 0, 7, 0),
             (TYPE_INT64, D_UNI, 0, 3, 0),
             (TYPE_INT64, D_UNI, 0, 1000, 0)]
    fns = [("row_number", -1), ("count_star", -1), ("min", 3)]
    n = 60_000
    t = eng.create_table(specs, n)
    try:
        eng.generate(t, SEED + 2)
        got = eng.window(t, fns, part_col=[0, 1, 2], order=[(3, 1, 1)])
    finally:
        t.free()
    cols, valids, types = gen(orc, specs, n, seed=SEED + 2)
    exp = orc.window(cols, valids, types, [(W[f[0]], f[1]) for f in fns],
                     part_col=[0, 1, 2], order=[(3, 1, 1)])
    assert got["n"] == exp["n"]
    assert np.array_equal(got["rowids"], exp["rowids"])
    assert np.array_equal(got["out_i"], exp["out_i"])

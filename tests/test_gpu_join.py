# GPU tests of the device equi-join (bkgpu_join / GpuEngine.join) against a
# brute-force numpy/dict join written here: key -> list of inner row ids,
# emitted in the contract's order (ascending outer row id, then ascending
# inner row id). A join moves values and computes nothing, so every cell,
# every null flag and the row order are compared bit-exactly.
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_agg import eng  # noqa: F401  (module-scoped fixture)

pytestmark = pytest.mark.gpu

I64, F64, STR, DT = 6, 12, 13, 14
HOWS = ("inner", "left", "semi", "anti")
KNOB = "BK_JOIN_LDS_KB"
LDS_KB = 128
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


@pytest.fixture(autouse=True)
def _clear_knob(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)


# ---- host side: tables and the reference join ------------------------------

class Side:
    """Host columns of one table + its device copy. cols: list of
    (type, data, valid-or-None); STR data is a list of str."""

    def __init__(self, eng, cols):
        self.eng = eng
        self.cols = [(t, (d if t == STR else np.ascontiguousarray(d)),
                      None if v is None else np.ascontiguousarray(v, np.uint8))
                     for t, d, v in cols]
        self.n = len(self.cols[0][1])
        self.types = [t for t, _, _ in self.cols]
        self.t = eng.create_table(
            [(t, 0, 0, 0, 0 if v is None else 1) for t, _, v in self.cols],
            self.n)
        for c, (t, d, v) in enumerate(self.cols):
            if t == STR:
                eng.upload_strings(self.t, c, d, v)
            else:
                eng.upload(self.t, c, d, v)

    def valid(self, c):
        v = self.cols[c][2]
        return np.ones(self.n, bool) if v is None else v.astype(bool)

    def bits(self, c):
        """Column as comparable 64-bit patterns (strings: the words)."""
        t, d, _ = self.cols[c]
        if t == STR:
            return np.array(d, dtype=object)
        return np.asarray(d).view(np.uint64) if t == F64 else \
            np.asarray(d, np.int64).view(np.uint64)

    def free(self):
        self.t.free()


def ref_pairs(outer, inner, on, how, opass=None, ipass=None):
    """(outer row ids, inner row ids or -1) in the contract's order."""
    opass = np.ones(outer.n, bool) if opass is None else opass
    ipass = np.ones(inner.n, bool) if ipass is None else ipass
    ok = [np.asarray(outer.cols[oc][1], np.int64) for oc, _ in on]
    ik = [np.asarray(inner.cols[ic][1], np.int64) for _, ic in on]
    ov = np.logical_and.reduce([outer.valid(oc) for oc, _ in on])
    iv = np.logical_and.reduce([inner.valid(ic) for _, ic in on])
    table = {}
    for r in np.nonzero(ipass & iv)[0]:
        table.setdefault(tuple(int(k[r]) for k in ik), []).append(int(r))
    orid, irid = [], []
    for r in np.nonzero(opass)[0]:
        m = table.get(tuple(int(k[r]) for k in ok), []) if ov[r] else []
        if how == "inner" or (how == "left" and m):
            orid += [r] * len(m)
            irid += m
        elif (how == "left") or (how == "semi" and m) or (how == "anti" and not m):
            orid.append(r)
            irid.append(-1)
    return np.array(orid, np.int64), np.array(irid, np.int64)


def fetch(eng, t):
    """Every column of a device table as (bits u64 | None, nulls)."""
    n = t.nrows
    ids = np.arange(max(n, 1), dtype=np.int64)
    out = []
    for c, ty in enumerate(t.col_types):
        vi = np.zeros(max(n, 1), np.int64)
        vd = np.zeros(max(n, 1), np.float64)
        nu = np.zeros(max(n, 1), np.uint8)
        if n:
            rc = eng.lib.bkgpu_gather(
                t.handle, c, ids.ctypes.data_as(C.POINTER(C.c_int64)), n,
                vi.ctypes.data_as(C.POINTER(C.c_int64)),
                vd.ctypes.data_as(C.POINTER(C.c_double)),
                nu.ctypes.data_as(C.POINTER(C.c_uint8)))
            assert rc == 0, eng.lib.bkgpu_last_error()
        bits = (vd if ty == F64 else vi).view(np.uint64)[:n].copy()
        out.append((bits, nu[:n].astype(bool)))
    return out


def check_result(eng, res, outer, inner, out, orid, irid):
    """Bit-exact comparison of a join result with the reference pairs."""
    assert res.nrows == len(orid), (res.nrows, len(orid))
    got = fetch(eng, res)
    assert len(got) == len(out)
    for c, (side, col) in enumerate(out):
        src, rid = (inner, irid) if side else (outer, orid)
        assert res.col_types[c] == src.types[col]
        none = rid < 0
        safe = np.where(none, 0, rid)
        if src.n == 0:
            exp_null = np.ones(len(rid), bool)
            exp = np.zeros(len(rid), np.uint64)
        else:
            exp_null = none | ~src.valid(col)[safe]
            exp = src.bits(col)[safe]
        bits, nulls = got[c]
        assert np.array_equal(nulls, exp_null), f"null flags of column {c}"
        live = ~exp_null
        if src.types[col] == STR:
            words = [eng.dict_word(res, c, int(code)) for code in bits[live]]
            assert words == list(exp[live]), f"words of column {c}"
        else:
            assert np.array_equal(bits[live], exp[live]), f"cells of column {c}"
        # a validity array is kept exactly where a NULL was written
        assert res.col_nullable[c] == bool(exp_null.any()), f"nullable {c}"
    return [(b.tobytes(), n.tobytes()) for b, n in got]


def default_out(outer, inner, how):
    out = [(0, c) for c in range(len(outer.types))]
    if how in ("inner", "left"):
        out += [(1, c) for c in range(len(inner.types))]
    return out


def both_routes(eng, monkeypatch, outer, inner, on, how, out=None,
                oplan=None, iplan=None, opass=None, ipass=None):
    """Run the join with the slot array probed from HBM/L2 and from LDS,
    check each against the reference and against each other."""
    orid, irid = ref_pairs(outer, inner, on, how, opass, ipass)
    cols = out if out is not None else default_out(outer, inner, how)
    snaps, stats = [], []
    for kb in (0, LDS_KB):
        monkeypatch.setenv(KNOB, str(kb))
        res = eng.join(outer.t, inner.t, on, how, out=out, outer_plan=oplan,
                       inner_plan=iplan)
        try:
            st = eng.join_stats()
            want = "lds" if kb and st["table_bytes"] <= kb * 1024 else "global"
            assert st["route"] == want, (kb, st)
            assert st["rows"] == len(orid)
            assert st["slots"] >= 2 * st["unique_keys"]
            assert st["slots"] & (st["slots"] - 1) == 0
            snaps.append(check_result(eng, res, outer, inner, cols, orid, irid))
            stats.append(st)
        finally:
            res.free()
    assert snaps[0] == snaps[1]
    return stats


def rng_of(seed):
    return np.random.default_rng(seed)


# ---- 1. tile and wave edges -------------------------------------------------

def _edge_sizes(eng):
    T = eng.join_tile_rows()
    return [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]


@pytest.mark.parametrize("which", range(8))
def test_tile_and_wave_edges(eng, monkeypatch, which):
    n = _edge_sizes(eng)[which]
    rng = rng_of(100 + which)
    ikeys = rng.permutation(2000)[:1000].astype(np.int64)   # 1000 unique keys
    inner = Side(eng, [(I64, ikeys, None),
                       (I64, rng.integers(-10**9, 10**9, 1000), None)])
    outer = Side(eng, [(I64, rng.integers(0, 2000, n), None),    # ~half absent
                       (I64, np.arange(n, dtype=np.int64) * 3, None)])
    try:
        for how in HOWS:
            st = both_routes(eng, monkeypatch, outer, inner, [(0, 0)], how)
            assert st[0]["unique_keys"] == 1000 and st[0]["outer_passed"] == n
            assert st[1]["route"] == "lds"
    finally:
        outer.free()
        inner.free()


# ---- 2. empty sides ---------------------------------------------------------

def test_empty_sides(eng, monkeypatch):
    from baikaldb_amd import QueryPlan
    rng = rng_of(2)
    outer = Side(eng, [(I64, rng.integers(0, 50, 300), None),
                       (I64, rng.integers(0, 10**6, 300), None)])
    inner = Side(eng, [(I64, np.arange(50, dtype=np.int64), None),
                       (I64, rng.integers(0, 10**6, 50), None)])
    far = Side(eng, [(I64, np.arange(1000, 1050, dtype=np.int64), None),
                     (I64, rng.integers(0, 10**6, 50), None)])
    none_o = QueryPlan(outer.types, conjuncts=[(1, "<", -1)])
    none_i = QueryPlan(inner.types, conjuncts=[(1, "<", -1)])
    no_o, no_i = np.zeros(outer.n, bool), np.zeros(inner.n, bool)
    try:
        for how in HOWS:
            kw = dict(on=[(0, 0)], how=how)
            # outer filter passes nothing
            both_routes(eng, monkeypatch, outer, inner, oplan=none_o,
                        opass=no_o, **kw)
            # inner filter passes nothing: INNER/SEMI empty, LEFT/ANTI all
            st = both_routes(eng, monkeypatch, outer, inner, iplan=none_i,
                             ipass=no_i, **kw)
            assert st[0]["rows"] == (0 if how in ("inner", "semi") else outer.n)
            assert st[0]["inner_passed"] == 0 and st[0]["unique_keys"] == 0
            # both empty
            both_routes(eng, monkeypatch, outer, inner, oplan=none_o,
                        iplan=none_i, opass=no_o, ipass=no_i, **kw)
            # no key in common
            st = both_routes(eng, monkeypatch, outer, far, **kw)
            assert st[0]["rows"] == (0 if how in ("inner", "semi") else outer.n)
            # every outer row matches
            st = both_routes(eng, monkeypatch, outer, inner, **kw)
            assert st[0]["rows"] == (0 if how == "anti" else outer.n)
    finally:
        outer.free()
        inner.free()
        far.free()


# ---- 3. N:M -----------------------------------------------------------------

def test_n_to_m(eng, monkeypatch):
    rng = rng_of(3)
    T = eng.join_tile_rows()
    mult = rng.integers(0, 6, 400)                      # 0..5 copies per key
    ikeys = np.repeat(np.arange(400, dtype=np.int64), mult)
    ikeys = np.concatenate([ikeys, np.full(3000, 777_777, np.int64)])
    rng.shuffle(ikeys)
    inner = Side(eng, [(I64, ikeys, None),
                       (I64, np.arange(len(ikeys), dtype=np.int64) + 10**6, None)])
    n = 2 * T + 300                                     # three tiles
    okeys = rng.integers(0, 500, n)
    okeys[rng.choice(n, 40, replace=False)] = 777_777   # ~40 rows hit the hot key
    outer = Side(eng, [(I64, okeys, None),
                       (I64, np.arange(n, dtype=np.int64), None)])
    try:
        for how in HOWS:
            st = both_routes(eng, monkeypatch, outer, inner, [(0, 0)], how)
        assert st[0]["unique_keys"] == int((mult > 0).sum()) + 1
    finally:
        outer.free()
        inner.free()


# ---- 4. keys that break sentinels and probing -------------------------------

@pytest.mark.parametrize("extra", [0, 1])
def test_sentinel_keys_and_table_doubling(eng, monkeypatch, extra):
    rng = rng_of(4 + extra)
    special = np.array([0, -1, I64_MIN, I64_MAX], np.int64)
    strided = (np.arange(1, 301, dtype=np.int64) << 20)     # multiples of 2^20
    nuniq = 1024 + extra                                    # 2^k / 2^k + 1
    neg = -rng.choice(np.arange(2, 10**6), nuniq - 304, replace=False)
    ikeys = np.concatenate([special, strided, neg.astype(np.int64)])
    assert len(np.unique(ikeys)) == nuniq
    ikeys = np.concatenate([ikeys, ikeys[:200]])            # some duplicates
    rng.shuffle(ikeys)
    inner = Side(eng, [(I64, ikeys, None),
                       (I64, rng.integers(I64_MIN, I64_MAX, len(ikeys)), None)])
    absent = np.array([1, -(1 << 20), I64_MIN + 1, I64_MAX - 1, 301 << 20],
                      np.int64)
    okeys = np.concatenate([special, special, strided, absent,
                            rng.choice(ikeys, 500), rng.integers(-50, 50, 200)])
    rng.shuffle(okeys)
    outer = Side(eng, [(I64, okeys, None)])
    try:
        for how in HOWS:
            st = both_routes(eng, monkeypatch, outer, inner, [(0, 0)], how)
            assert st[0]["unique_keys"] == nuniq
            # load <= 1/2: 2^k keys fill 2^(k+1) slots, one more key doubles
            assert st[0]["slots"] == (2048 if extra == 0 else 4096)
    finally:
        outer.free()
        inner.free()


# ---- 5. NULL keys -----------------------------------------------------------

def test_null_keys(eng, monkeypatch):
    rng = rng_of(5)
    no, ni = 3000, 800
    ov = (rng.random(no) >= 0.1).astype(np.uint8)
    iv = (rng.random(ni) >= 0.1).astype(np.uint8)
    ov[0] = 0
    iv[:3] = 0                          # NULL-key inner rows exist
    okeys = rng.integers(0, 300, no)
    ikeys = rng.integers(0, 300, ni)
    okeys[0] = ikeys[0]                 # outer NULL key "equal" to an inner NULL key
    outer = Side(eng, [(I64, okeys, ov), (I64, np.arange(no, dtype=np.int64), None)])
    inner = Side(eng, [(I64, ikeys, iv), (I64, np.arange(ni, dtype=np.int64), None)])
    try:
        for how in HOWS:
            st = both_routes(eng, monkeypatch, outer, inner, [(0, 0)], how)
            assert st[0]["inner_passed"] == int(iv.sum())
    finally:
        outer.free()
        inner.free()


# ---- 6. two key columns -----------------------------------------------------

def test_two_key_columns(eng, monkeypatch):
    rng = rng_of(6)
    no, ni = 2500, 600
    # small domains: many pairs agree on one key and differ on the other
    oa, ob = rng.integers(0, 12, no), rng.integers(-6, 6, no)
    ia, ib = rng.integers(0, 12, ni), rng.integers(-6, 6, ni)
    ova = np.ones(no, np.uint8); ovb = np.ones(no, np.uint8)
    iva = np.ones(ni, np.uint8); ivb = np.ones(ni, np.uint8)
    ova[5] = 0; ovb[9] = 0; iva[2] = 0; ivb[4] = 0      # one NULL in either column
    outer = Side(eng, [(I64, oa, ova), (I64, ob, ovb),
                       (I64, np.arange(no, dtype=np.int64), None)])
    inner = Side(eng, [(I64, ib, ivb), (I64, ia, iva),
                       (I64, np.arange(ni, dtype=np.int64) * 7, None)])
    try:
        for how in HOWS:
            both_routes(eng, monkeypatch, outer, inner, [(0, 1), (1, 0)], how)
    finally:
        outer.free()
        inner.free()


def test_datetime_keys(eng, monkeypatch):
    rng = rng_of(61)
    base = (2024 * 13 + 5) << 46
    outer = Side(eng, [(DT, base + (rng.integers(1, 28, 500) << 41), None)])
    inner = Side(eng, [(DT, base + (rng.integers(1, 20, 40) << 41), None),
                       (I64, np.arange(40, dtype=np.int64), None)])
    try:
        both_routes(eng, monkeypatch, outer, inner, [(0, 0)], "left")
    finally:
        outer.free()
        inner.free()


# ---- 7. column forms --------------------------------------------------------

def test_column_forms(eng, monkeypatch):
    rng = rng_of(7)
    no, ni = 1500, 200
    dbl = rng.standard_normal(ni)
    dbl[:4] = [np.nan, -0.0, 0.0, np.inf]
    pv = (rng.random(ni) >= 0.2).astype(np.uint8)
    words = [f"w{int(x):03d}" for x in rng.integers(0, 40, ni)]
    wv = (rng.random(ni) >= 0.1).astype(np.uint8)
    inner = Side(eng, [(I64, rng.permutation(ni).astype(np.int64) + 1000, None),
                       (I64, rng.integers(0, 200, ni), None),       # narrow payload
                       (F64, dbl, None),
                       (I64, rng.integers(I64_MIN, I64_MAX, ni), pv),
                       (STR, words, wv)])
    outer = Side(eng, [(I64, rng.integers(1000, 1000 + ni, no), None),
                       (I64, rng.integers(-100, 100, no), None)])
    try:
        eng.compact(inner.t)
        eng.compact(outer.t)
        assert eng.col_width(inner.t, 0) < 8 and eng.col_width(inner.t, 1) < 8
        assert eng.col_width(outer.t, 0) < 8 and eng.col_width(outer.t, 1) < 8
        for how in HOWS:
            both_routes(eng, monkeypatch, outer, inner, [(0, 0)], how)
        # nullability: a NULL-free INNER result keeps no validity array
        res = eng.join(outer.t, inner.t, [(0, 0)], "inner",
                       out=[(0, 0), (0, 1), (1, 1), (1, 2)])
        assert res.nrows == no and res.col_nullable == [False] * 4
        assert all(eng.lib.bkgpu_table_col_nullable(res.handle, c) == 0
                   for c in range(4))
        res.free()
    finally:
        outer.free()
        inner.free()
    # a LEFT result with an unmatched row: inner columns only are nullable
    outer = Side(eng, [(I64, np.array([1, 2, 3], np.int64), None)])
    inner = Side(eng, [(I64, np.array([1, 3], np.int64), None),
                       (I64, np.array([10, 30], np.int64), None)])
    try:
        res = eng.join(outer.t, inner.t, [(0, 0)], "left")
        assert [eng.lib.bkgpu_table_col_nullable(res.handle, c)
                for c in range(3)] == [0, 1, 1]
        res.free()
    finally:
        outer.free()
        inner.free()


# ---- 8. side filters --------------------------------------------------------

def test_side_filters(eng, monkeypatch):
    from baikaldb_amd import QueryPlan
    rng = rng_of(8)
    no, ni = 4000, 500
    outer = Side(eng, [(I64, rng.integers(0, 600, no), None),
                       (I64, rng.integers(0, 100, no), None)])
    inner = Side(eng, [(I64, rng.integers(0, 600, ni), None),
                       (I64, rng.integers(0, 10**4, ni), None)])
    oa = np.asarray(outer.cols[1][1])
    ia = np.asarray(inner.cols[1][1])
    try:
        for how in HOWS:
            # a plain conjunct on each side
            both_routes(eng, monkeypatch, outer, inner, [(0, 0)], how,
                        oplan=QueryPlan(outer.types, conjuncts=[(1, "<", 40)]),
                        iplan=QueryPlan(inner.types, conjuncts=[(1, ">=", 2000)]),
                        opass=oa < 40, ipass=ia >= 2000)
            # an expression program on the inner side: a % 7 = 0
            st = both_routes(
                eng, monkeypatch, outer, inner, [(0, 0)], how,
                iplan=QueryPlan(inner.types,
                                conjuncts=[(("mod", 1, ("liti", 7)), "=", 0)]),
                ipass=ia % 7 == 0)
            assert st[0]["inner_passed"] == int((ia % 7 == 0).sum())
    finally:
        outer.free()
        inner.free()


# ---- 9. routes: a table too large for the knob stays global -----------------

def test_large_table_reports_global_route(eng, monkeypatch):
    rng = rng_of(9)
    ikeys = rng.permutation(20000)[:5000].astype(np.int64)   # 16384 slots = 256 KB
    inner = Side(eng, [(I64, ikeys, None)])
    outer = Side(eng, [(I64, rng.integers(0, 20000, 3000), None)])
    try:
        st = both_routes(eng, monkeypatch, outer, inner, [(0, 0)], "inner")
        assert st[1]["table_bytes"] > LDS_KB * 1024
        assert [s["route"] for s in st] == ["global", "global"]
    finally:
        outer.free()
        inner.free()


def test_default_route_threshold(eng):
    """Knob unset: slot arrays up to the measured 64 KB crossover (DESIGN.md
    §4) are probed from LDS, larger ones from HBM/L2."""
    rng = rng_of(91)
    outer = Side(eng, [(I64, rng.integers(0, 9000, 5000), None)])
    try:
        for nkeys, route in ((2048, "lds"), (2049, "global")):
            inner = Side(eng, [(I64, rng.permutation(9000)[:nkeys].astype(np.int64),
                                None)])
            try:
                res = eng.join(outer.t, inner.t, [(0, 0)], "inner")
                st = eng.join_stats()
                orid, irid = ref_pairs(outer, inner, [(0, 0)], "inner")
                check_result(eng, res, outer, inner, [(0, 0), (1, 0)], orid, irid)
                res.free()
                assert st["table_bytes"] == (65536 if route == "lds" else 131072)
                assert st["route"] == route, st
            finally:
                inner.free()
    finally:
        outer.free()


# ---- 10. right join ---------------------------------------------------------

def test_right_equals_swapped_left(eng):
    rng = rng_of(10)
    a = Side(eng, [(I64, rng.integers(0, 80, 700), None),
                   (I64, np.arange(700, dtype=np.int64), None)])
    b = Side(eng, [(I64, rng.integers(0, 120, 300), None),
                   (F64, rng.standard_normal(300), None)])
    try:
        # a RIGHT JOIN b keeps every b row; columns stay (a..., b...)
        right = eng.join(a.t, b.t, [(0, 0)], "right")
        left = eng.join(b.t, a.t, [(0, 0)], "left",
                        out=[(1, 0), (1, 1), (0, 0), (0, 1)])
        try:
            assert right.col_types == left.col_types == [I64, I64, I64, F64]
            assert right.nrows == left.nrows
            gr, gl = fetch(eng, right), fetch(eng, left)
            for (br, nr), (bl, nl) in zip(gr, gl):
                assert np.array_equal(nr, nl)
                assert np.array_equal(br[~nr], bl[~nl])
            orid, irid = ref_pairs(b, a, [(0, 0)], "left")
            check_result(eng, right, b, a, [(1, 0), (1, 1), (0, 0), (0, 1)],
                         orid, irid)
        finally:
            right.free()
            left.free()
    finally:
        a.free()
        b.free()


# ---- 11. downstream operators over joined rows ------------------------------

def test_downstream_operators(eng):
    """SELECT d.attr, COUNT(*), SUM(f.v), MIN(f.v) FROM f JOIN d ON f.k = d.k
    WHERE f.a < K GROUP BY d.attr — join, then filter_agg over the join."""
    from baikaldb_amd import QueryPlan
    rng = rng_of(11)
    nf, nd, K = 200_000, 1000, 60
    fk = rng.integers(0, 1100, nf)                        # ~9% miss the dimension
    fv = rng.integers(-10**6, 10**6, nf)
    fa = rng.integers(0, 100, nf)
    dk = rng.permutation(nd).astype(np.int64)
    dattr = rng.integers(0, 25, nd)
    f = Side(eng, [(I64, fk, None), (I64, fv, None), (I64, fa, None)])
    d = Side(eng, [(I64, dk, None), (I64, dattr, None)])
    try:
        j = eng.join(f.t, d.t, [(0, 0)], "inner",
                     out=[(0, 0), (0, 1), (0, 2), (1, 1)])
        try:
            attr_of = np.full(1100, -1, np.int64)
            attr_of[dk] = dattr
            hit = attr_of[fk] >= 0
            jv, ja, jattr = fv[hit], fa[hit], attr_of[fk][hit]
            assert j.nrows == int(hit.sum())
            assert j.col_nullable == [False] * 4
            # GROUP BY the dimension attribute
            plan = QueryPlan(j.col_types, conjuncts=[(2, "<", K)], group=[3],
                             aggs=[("count_star", -1), ("sum", 1), ("min", 1)])
            res = eng.filter_agg(j, plan)
            gt = res.to_table(canonical=True)
            got = fetch(eng, gt)
            gt.free()
            res.free()
            keep = ja < K
            attrs = np.unique(jattr[keep])
            assert np.array_equal(got[0][0].view(np.int64), attrs)
            for g, a in enumerate(attrs):
                sel = keep & (jattr == a)
                assert got[1][0].view(np.int64)[g] == sel.sum()
                assert got[2][0].view(np.int64)[g] == jv[sel].sum()
                assert got[3][0].view(np.int64)[g] == jv[sel].min()
            # top-N on a joined column (ties fall in arrival order)
            top = eng.sort_topk(j, [(1, 1, 0)], 10)
            assert np.array_equal(top, np.argsort(jv, kind="stable")[:10])
            # an expression over one outer and one inner column
            c = eng.derive_expr(j, ("add", 1, 3))
            col = fetch(eng, j)[c]
            assert not col[1].any()
            assert np.array_equal(col[0].view(np.int64), jv + jattr)
        finally:
            j.free()
    finally:
        f.free()
        d.free()


# ---- 12. size guard ---------------------------------------------------------

def test_result_size_guard(eng):
    n = 50_000
    one = np.full(n, 42, np.int64)
    a = Side(eng, [(I64, one, None)])
    b = Side(eng, [(I64, one, None)])
    try:
        with pytest.raises(RuntimeError, match=r"2\^31"):
            eng.join(a.t, b.t, [(0, 0)], "inner")       # 2.5e9 pairs
        # SEMI over the same tables is small, and the engine is still usable
        res = eng.join(a.t, b.t, [(0, 0)], "semi")
        assert res.nrows == n
        res.free()
    finally:
        a.free()
        b.free()
    small_o = Side(eng, [(I64, np.array([3, 1, 2, 1], np.int64), None)])
    small_i = Side(eng, [(I64, np.array([1, 1, 3], np.int64), None)])
    try:
        res = eng.join(small_o.t, small_i.t, [(0, 0)], "inner")
        orid, irid = ref_pairs(small_o, small_i, [(0, 0)], "inner")
        assert list(orid) == [0, 1, 1, 3, 3] and list(irid) == [2, 0, 1, 0, 1]
        check_result(eng, res, small_o, small_i, [(0, 0), (1, 0)], orid, irid)
        res.free()
    finally:
        small_o.free()
        small_i.free()


# ---- 13. rejections ---------------------------------------------------------

def test_rejections(eng):
    from baikaldb_amd.plan import BkJoinSpec
    t = Side(eng, [(I64, np.arange(8, dtype=np.int64), None),
                   (F64, np.arange(8, dtype=np.float64), None),
                   (STR, [f"s{i}" for i in range(8)], None),
                   (DT, np.arange(8, dtype=np.int64) << 41, None)])

    def spec(jt, keys, out):
        s = BkJoinSpec()
        s.join_type, s.n_keys, s.n_out = jt, len(keys), len(out)
        for i, (oc, ic) in enumerate(keys[:2]):
            s.outer_key[i], s.inner_key[i] = oc, ic
        for i, (side, col) in enumerate(out[:16]):
            s.out_side[i], s.out_col[i] = side, col
        return s

    ok_out = [(0, 0), (1, 0)]
    bad = {
        "double key": spec(3, [(1, 1)], ok_out),
        "string key": spec(3, [(2, 2)], ok_out),
        "int64 vs datetime": spec(3, [(0, 3)], ok_out),
        "0 key pairs": spec(3, [], ok_out),
        "3 key pairs": spec(3, [(0, 0), (0, 0), (0, 0)], ok_out),
        "n_out too large": spec(3, [(0, 0)], [(0, 0)] * 17),
        "inner column under semi": spec(4, [(0, 0)], ok_out),
        "full join": spec(6, [(0, 0)], ok_out),
        "null join": spec(0, [(0, 0)], ok_out),
        "right join in the kernel": spec(2, [(0, 0)], ok_out),
    }
    try:
        for what, s in bad.items():
            h = eng.lib.bkgpu_join(t.t.handle, None, t.t.handle, None, C.byref(s))
            assert not h, what
            msg = eng.lib.bkgpu_last_error().decode()
            assert msg.startswith("join:"), (what, msg)
        # the engine is unharmed
        res = eng.join(t.t, t.t, [(0, 0)], "inner", out=ok_out)
        assert res.nrows == 8
        res.free()
    finally:
        t.free()


# ---- 14. repeatability ------------------------------------------------------

def test_repeatable(eng):
    rng = rng_of(14)
    outer = Side(eng, [(I64, rng.integers(0, 300, 9000), None),
                       (F64, rng.standard_normal(9000), None)])
    inner = Side(eng, [(I64, rng.integers(0, 300, 1200), None),
                       (I64, rng.integers(0, 10**9, 1200), None)])
    try:
        snaps = []
        for _ in range(3):
            res = eng.join(outer.t, inner.t, [(0, 0)], "left")
            snaps.append([(b.tobytes(), n.tobytes()) for b, n in fetch(eng, res)])
            res.free()
        assert snaps[0] == snaps[1] == snaps[2]
    finally:
        outer.free()
        inner.free()

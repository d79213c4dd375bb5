# Divide / mod / unary minus / compares and the conditional family (if,
# ifnull, nullif, isnull, CASE) in the engine's postfix expression programs
# (eval_prog in bkgpu.hip), through every consumer of an expression slot:
# derived columns, WHERE conjuncts (eager slots, the lazy >4 loop and OR
# groups), aggregate inputs (fused and partitioned routes), GROUP BY and
# ORDER BY over derived columns, and the host validators.
#
# Reference: the numpy interpreter tests/_exprref.py (itself checked against
# hand-derived vectors by tests/test_expr_cond_plan.py). Parity is bit-exact
# for int64 and f64 values and for nullness: the build has no fast-math, so
# the f64 divide is the correctly rounded IEEE quotient, equal to numpy's.
# The only tolerance is on DOUBLE SUM/AVG, whose reduction order differs:
# the repository's 1e-9 * (sum|x| + 1), as in test_derive_expr.py.
#
# Tables have N = 4099 rows (not a multiple of 64 or 256; the work is per
# row) plus one case at N = 1. Inputs: ~20 % NULLs, zeros forced into ~10 %
# of the divisors (-0.0 among the double ones), and the INT64 extremes.
import ctypes as C

import numpy as np
import pytest

from tests import _exprref as R

pytestmark = pytest.mark.gpu

TYPE_INT64, TYPE_DOUBLE = 6, 12
N = 4099
SEED = 0xC04D
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max

# column layout of the shared data set
RID, A, B, X, Y, G, CC, V = range(8)


@pytest.fixture(scope="module")
def eng():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    from baikaldb_amd import GpuEngine
    return GpuEngine()


def _make_data(n, seed=SEED):
    rng = np.random.default_rng(seed)
    a = rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)
    b = rng.integers(-3, 4, n, dtype=np.int64)
    b[rng.random(n) < 0.10] = 0
    x = rng.standard_normal(n)
    y = rng.standard_normal(n)
    zy = rng.random(n) < 0.10
    y[zy] = np.where(rng.random(int(zy.sum())) < 0.5, 0.0, -0.0)
    if n >= 16:
        # INT64 extremes, on both sides of mod / under neg
        a[:4] = [I64_MIN, I64_MIN, I64_MAX, I64_MIN]
        b[:4] = [-1, 1, -1, I64_MIN]
        a[4:6] = [7, -7]
        b[4:6] = [I64_MAX, I64_MIN]
    cols = [np.arange(n, dtype=np.int64), a, b, x, y,
            rng.integers(0, 7, n, dtype=np.int64),
            rng.integers(-3, 4, n, dtype=np.int64),
            rng.integers(0, 1000, n, dtype=np.int64)]
    valids = [None,
              (rng.random(n) > 0.2).astype(np.uint8),
              (rng.random(n) > 0.2).astype(np.uint8),
              (rng.random(n) > 0.2).astype(np.uint8),
              (rng.random(n) > 0.2).astype(np.uint8),
              None,
              (rng.random(n) > 0.2).astype(np.uint8),
              None]
    if n >= 16:
        for c in (A, B):
            valids[c][:6] = 1          # the extreme rows stay non-NULL
    return cols, valids


@pytest.fixture(scope="module")
def data():
    return _make_data(N)


def _upload(eng, cols, valids):
    specs = [(TYPE_DOUBLE if c.dtype == np.float64 else TYPE_INT64, 0, 0,
              1 << 31, 1 if v is not None else 0)
             for c, v in zip(cols, valids)]
    t = eng.create_table(specs, len(cols[0]))
    for i, (c, v) in enumerate(zip(cols, valids)):
        eng.upload(t, i, np.ascontiguousarray(c), v)
    return t


def _derived_rows(eng, cols, valids, expr):
    """derive_expr(expr), then GROUP BY the unique row id with MIN and COUNT
    of the derived column: one group per row carries the row's value and
    nullness back. Returns (domain, valid[n], value[n])."""
    from baikaldb_amd import QueryPlan
    n = len(cols[0])
    t = _upload(eng, cols, valids)
    try:
        nc = eng.derive_expr(t, expr)
        dom = t.col_types[nc]
        plan = QueryPlan(t.col_types, group=[RID],
                         aggs=[("min", nc), ("count", nc)])
        res = eng.filter_agg(t, plan, expected_groups=n)
        got = res.fetch(sorted=True)
        res.free()
    finally:
        t.free()
    assert got["ngroups"] == n and got["rows_passed"] == n
    rid = (got["enc"][:, 0] ^ np.uint64(1 << 63)).astype(np.int64)
    assert np.array_equal(rid, np.arange(n))
    has = got["agg_has"][0].astype(bool)
    assert np.array_equal(got["agg_i"][1], has.astype(np.int64))
    val = got["agg_d"][0] if dom == TYPE_DOUBLE else got["agg_i"][0]
    return dom, has, val


def _assert_rows_equal(dom, has, val, rdom, rv, rx):
    assert dom == rdom
    print(f"rows {len(rv)}: non-NULL expected {int(rv.sum())}, "
          f"got {int(has.sum())}")
    assert np.array_equal(has, rv)
    bad = np.flatnonzero(val.view(np.int64)[rv] != rx.view(np.int64)[rv])
    print(f"value bit mismatches: {len(bad)}")
    assert len(bad) == 0, (val[rv][bad[:5]], rx[rv][bad[:5]])


_GT0 = ("gt", CC, ("liti", 0))
_LT0 = ("lt", CC, ("liti", 0))
PER_ROW = {
    "div_int": ("div", A, B),
    "div_double": ("div", X, Y),
    "mod": ("mod", A, B),
    "neg_int": ("neg", A),
    "neg_double": ("neg", X),
    "if_mixed": ("if", _GT0, A, X),
    "if_double_cond": ("if", Y, A, ("liti", -1)),
    "ifnull": ("ifnull", A, B),
    "nullif": ("nullif", CC, B),
    "isnull": ("isnull", X),
    "case_else": ("case", [(_GT0, A), (_LT0, ("neg", A))], ("liti", 30)),
    "case_no_else": ("case", [(_GT0, A), (_LT0, X)], None),
    "case_expr": ("case_expr", CC, [(("liti", 1), A), (B, X)], None),
    # operand stack depth 5: isnull | neg | a | b | 3
    "nested_depth5": ("if", ("isnull", A), ("neg", B),
                      ("add", ("mod", A, ("ifnull", B, ("liti", 3))), B)),
}


@pytest.mark.parametrize("name", list(PER_ROW))
def test_per_row_parity(eng, data, name):
    cols, valids = data
    expr = PER_ROW[name]
    rdom, rv, rx = R.eval_expr(expr, cols, valids)
    dom, has, val = _derived_rows(eng, cols, valids, expr)
    _assert_rows_equal(dom, has, val, rdom, rv, rx)


@pytest.mark.parametrize("row", [
    # (a, a_valid, b, b_valid)
    (I64_MIN, 1, -1, 1), (5, 1, 0, 1), (5, 0, 2, 1)])
def test_single_row_table(eng, row):
    """n = 1: mod and divide on a one-row table."""
    a, va, b, vb = row
    cols, valids = _make_data(1)
    cols[A][:], cols[B][:] = a, b
    valids[A][:], valids[B][:] = va, vb
    for expr in (("mod", A, B), ("div", A, B)):
        rdom, rv, rx = R.eval_expr(expr, cols, valids)
        dom, has, val = _derived_rows(eng, cols, valids, expr)
        _assert_rows_equal(dom, has, val, rdom, rv, rx)


def test_validity_materialized_for_non_nullable_inputs(eng):
    """Non-nullable a and b, zeros in b: a % b is NULL on those rows, so the
    derived column needs a validity vector of its own — COUNT(derived) must
    equal the number of nonzero b, not the row count."""
    from baikaldb_amd import QueryPlan
    rng = np.random.default_rng(SEED + 1)
    a = rng.integers(-1000, 1000, N, dtype=np.int64)
    b = rng.integers(-5, 6, N, dtype=np.int64)
    t = _upload(eng, [a, b], [None, None])
    try:
        nm = eng.derive_expr(t, ("mod", 0, 1))
        nd = eng.derive_expr(t, ("div", 0, 1))
        res = eng.filter_agg(t, QueryPlan(
            t.col_types, aggs=[("count", nm), ("count", nd), ("sum", nm),
                               ("count_star", -1)]))
        got = res.fetch()
        res.free()
    finally:
        t.free()
    nz = b != 0
    assert 0 < nz.sum() < N
    assert got["agg_i"][3][0] == N
    assert got["agg_i"][0][0] == int(nz.sum())
    assert got["agg_i"][1][0] == int(nz.sum())
    assert got["agg_i"][2][0] == int(np.fmod(a[nz], b[nz]).sum())


# ---- as a predicate ----------------------------------------------------

PREDS = {
    "mod7_eq_0": (("mod", A, ("liti", 7)), "=", 0),
    "div_gt_half": (("div", A, B), ">", 0.5),
    "if_isnull_eq_1": (("if", ("isnull", A), ("liti", 1), ("liti", 0)),
                       "=", 1),
}


def _pred_mask(cols, valids, pred):
    expr, op, lit = pred
    _, v, x = R.eval_expr(expr, cols, valids)
    with np.errstate(invalid="ignore"):
        hit = {"=": x == lit, ">": x > lit}[op]
    return v & hit


@pytest.mark.parametrize("where", ["conjunct0", "conjunct4", "or_group"])
@pytest.mark.parametrize("name", list(PREDS))
def test_predicate(eng, data, name, where):
    """The same program predicate in an eager slot (conjunct 0), in the
    lazy loop that evaluates conjuncts past the first four (index 4), and
    as a member of an OR clause (v < 100 OR pred)."""
    from baikaldb_amd import QueryPlan
    cols, valids = data
    pred = PREDS[name]
    mask = _pred_mask(cols, valids, pred)
    if where == "conjunct0":
        conj = [pred]
    elif where == "conjunct4":
        conj = [(RID, ">=", 0), (V, ">=", 0), (G, "<", 7), (RID, "<", N),
                pred]
    else:
        conj = [(V, "<", 100, 1), pred + (1,)]
        mask = mask | (cols[V] < 100)
    t = _upload(eng, cols, valids)
    try:
        plan = QueryPlan(t.col_types, conjuncts=conj,
                         aggs=[("count_star", -1), ("sum", V), ("count", A)])
        res = eng.filter_agg(t, plan)
        got = res.fetch()
        res.free()
    finally:
        t.free()
    print(f"rows_passed expected {int(mask.sum())}, got {got['rows_passed']}")
    assert 0 < mask.sum() < N
    assert got["rows_passed"] == int(mask.sum())
    assert got["agg_i"][0][0] == int(mask.sum())
    assert got["agg_i"][1][0] == int(cols[V][mask].sum())
    assert got["agg_i"][2][0] == int((valids[A].astype(bool) & mask).sum())


# ---- as an aggregate input ---------------------------------------------

_SUM_IF = ("if", ("gt", CC, ("liti", 0)), V, ("liti", 0))
_AVG_IFNULL = ("ifnull", X, ("liti", 0))


def _group_ref(cols, valids, expr):
    _, v, x = R.eval_expr(expr, cols, valids)
    return v, x


def _run_grouped(eng, cols, valids, aggs, expected_groups):
    from baikaldb_amd import QueryPlan
    t = _upload(eng, cols, valids)
    try:
        plan = QueryPlan(t.col_types, group=[G], aggs=aggs)
        res = eng.filter_agg(t, plan, expected_groups=expected_groups)
        got = res.fetch(sorted=True)
        res.free()
    finally:
        t.free()
    keys = (got["enc"][:, 0] ^ np.uint64(1 << 63)).astype(np.int64)
    assert np.array_equal(keys, np.arange(7))
    return got


def test_aggregate_inputs_seven_groups(eng, data):
    """SUM(if(c > 0, v, 0)) — int64, bit-exact — and AVG(ifnull(x, 0)) —
    f64 within 1e-9 * (sum|x| + 1) on the sum — over 7 groups."""
    cols, valids = data
    got = _run_grouped(eng, cols, valids,
                       [("sum", _SUM_IF), ("avg", _AVG_IFNULL),
                        ("sum", _AVG_IFNULL), ("count", _AVG_IFNULL)], 16)
    vi, xi = _group_ref(cols, valids, _SUM_IF)
    vd, xd = _group_ref(cols, valids, _AVG_IFNULL)
    assert vi.all() and vd.all()       # neither expression can be NULL
    for g in range(7):
        m = cols[G] == g
        assert got["agg_i"][0][g] == int(xi[m].sum())
        tol = 1e-9 * (np.abs(xd[m]).sum() + 1)
        err_sum = abs(got["agg_d"][2][g] - xd[m].sum())
        err_avg = abs(got["agg_d"][1][g] - xd[m].sum() / m.sum()) * m.sum()
        print(f"group {g}: sum err {err_sum:.3e} avg err*n {err_avg:.3e} "
              f"tol {tol:.3e}")
        assert err_sum <= tol and err_avg <= tol
        assert got["agg_i"][3][g] == int(m.sum())


@pytest.mark.parametrize("sorted_range", [None, "0"])
def test_aggregate_input_partitioned_route(eng, data, monkeypatch,
                                           sorted_range):
    """The integer query again with a large expected_groups: the engine
    leaves the fused kernel for its partitioned routes (sort-dedup by
    default; BK_SORTED_RANGE=0 keeps it on the hash-partitioned pipeline).
    Same answer on every route."""
    if sorted_range is not None:
        monkeypatch.setenv("BK_SORTED_RANGE", sorted_range)
    cols, valids = data
    aggs = [("sum", _SUM_IF), ("count", ("nullif", CC, B)),
            ("min", ("mod", A, B))]
    got = _run_grouped(eng, cols, valids, aggs, 1 << 16)
    fused = _run_grouped(eng, cols, valids, aggs, 16)
    _, xi = _group_ref(cols, valids, _SUM_IF)
    vn, _ = _group_ref(cols, valids, ("nullif", CC, B))
    vm, xm = _group_ref(cols, valids, ("mod", A, B))
    for g in range(7):
        m = cols[G] == g
        assert got["agg_i"][0][g] == int(xi[m].sum())
        assert got["agg_i"][1][g] == int(vn[m].sum())
        assert got["agg_i"][2][g] == int(xm[m & vm].min())
    assert np.array_equal(got["agg_i"], fused["agg_i"])
    assert np.array_equal(got["agg_has"], fused["agg_has"])


# ---- other consumers ---------------------------------------------------

def test_group_by_derived_case_bucket(eng, data):
    """GROUP BY CASE WHEN c > 0 THEN 1 WHEN c < 0 THEN -1 ELSE 0 END (a NULL
    c falls to ELSE) through a derived column."""
    from baikaldb_amd import QueryPlan
    cols, valids = data
    bucket = ("case", [(_GT0, ("liti", 1)), (_LT0, ("liti", -1))],
              ("liti", 0))
    _, bv, bx = R.eval_expr(bucket, cols, valids)
    assert bv.all()
    t = _upload(eng, cols, valids)
    try:
        nc = eng.derive_expr(t, bucket)
        plan = QueryPlan(t.col_types, group=[nc],
                         aggs=[("count_star", -1), ("sum", V)])
        res = eng.filter_agg(t, plan, expected_groups=16)
        got = res.fetch(sorted=True)
        res.free()
    finally:
        t.free()
    assert got["ngroups"] == 3
    keys = (got["enc"][:, 0] ^ np.uint64(1 << 63)).astype(np.int64)
    assert list(keys) == [-1, 0, 1]
    for k, key in enumerate(keys):
        m = bx == key
        assert got["agg_i"][0][k] == int(m.sum())
        assert got["agg_i"][1][k] == int(cols[V][m].sum())


def test_sort_topk_by_derived_neg_with_program_conjunct(eng, data):
    """ORDER BY -a (NULLs first) LIMIT 400 WHERE v % 3 = 0: the row ids equal
    numpy's stable argsort. The limit reaches past the ~270 NULL rows into
    the values, where -INT64_MIN wraps to INT64_MIN and sorts first."""
    from baikaldb_amd import QueryPlan
    cols, valids = data
    _, nv, nx = R.eval_expr(("neg", A), cols, valids)
    passed = np.flatnonzero(cols[V] % 3 == 0)
    key = np.where(nv, nx, 0)
    order = np.lexsort((passed, key[passed], nv[passed]))
    expect = passed[order][:400]
    assert nv[expect].any() and not nv[expect].all()
    t = _upload(eng, cols, valids)
    try:
        nc = eng.derive_expr(t, ("neg", A))
        plan = QueryPlan(t.col_types,
                         conjuncts=[(("mod", V, ("liti", 3)), "=", 0)])
        rowids = eng.sort_topk(t, [(nc, 1, 1)], 400, plan=plan)
    finally:
        t.free()
    assert np.array_equal(np.asarray(rowids), expect)


# ---- rejection, through bkgpu_last_error --------------------------------

def _op(**kw):
    from baikaldb_amd.plan import BkExprOp
    o = BkExprOp()
    o.domain = TYPE_INT64
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _filter_agg_error(eng, t, ops, arith=0):
    """Run a COUNT(*) whose conjunct 0 carries `ops` (or the legacy arith
    slot); returns bkgpu_last_error() after the expected refusal."""
    from baikaldb_amd import QueryPlan
    q = QueryPlan(t.col_types, conjuncts=[(0, "=", 0)],
                  aggs=[("count_star", -1)]).to_spec()
    cj = q.conjuncts[0]
    if arith:
        cj.arith, cj.col2 = arith, 1
    for k, o in enumerate(ops):
        q.prog[k] = o
    q.n_prog = len(ops)
    cj.prog_begin, cj.prog_len = 0, len(ops)
    h = eng.lib.bkgpu_filter_agg(t.handle, C.byref(q), 0, t.nrows, 16)
    if h:
        eng.lib.bkgpu_agg_free(h)
    assert not h, "the validator accepted a bad query"
    return eng.lib.bkgpu_last_error().decode()


def _derive_error(eng, t, ops, out_type=TYPE_INT64):
    from baikaldb_amd.plan import BkExprOp
    arr = (BkExprOp * len(ops))(*ops)
    rc = eng.lib.bkgpu_table_derive_prog(t.handle, C.cast(arr, C.c_void_p),
                                         len(ops), out_type)
    assert rc < 0, "the validator accepted a bad program"
    return eng.lib.bkgpu_last_error().decode()


BAD_PROGRAMS = {
    "int64_divide": ([dict(op=R.COL, arg=0), dict(op=R.COL, arg=1),
                      dict(op=R.ARITH, arg=R.DIV, domain=TYPE_INT64)],
                     "DOUBLE"),
    "double_mod": ([dict(op=R.COL, arg=0), dict(op=R.COL, arg=1),
                    dict(op=R.ARITH, arg=R.MOD, domain=TYPE_DOUBLE)],
                   "INT64"),
    "if_underflow": ([dict(op=R.COL, arg=0), dict(op=R.COL, arg=1),
                      dict(op=R.IF)], "underflow"),
    "opcode_99": ([dict(op=R.COL, arg=0), dict(op=99)], "opcode"),
    "cmp_arg_in": ([dict(op=R.COL, arg=0), dict(op=R.COL, arg=1),
                    dict(op=R.CMP, arg=6)], "compare"),
}


@pytest.fixture(scope="module")
def small_table(eng):
    a = np.arange(64, dtype=np.int64)
    t = _upload(eng, [a, a.copy()], [None, None])
    yield t
    t.free()


@pytest.mark.parametrize("name", list(BAD_PROGRAMS))
def test_validators_reject(eng, small_table, name):
    ops, word = BAD_PROGRAMS[name]
    ops = [_op(**o) for o in ops]
    err = _filter_agg_error(eng, small_table, ops)
    assert "program" in err and word in err, err
    err = _derive_error(eng, small_table, ops)
    assert err.startswith("derive_prog") and word in err, err


def test_legacy_arith_slot_rejects_mod(eng, small_table):
    """BkConjunct.arith / BkAggSpec.arith decode as ADD ? : SUB ? : MUL in
    the kernels: a MOD there would silently multiply, so it is refused."""
    from baikaldb_amd import QueryPlan
    err = _filter_agg_error(eng, small_table, [], arith=R.MOD)
    assert "arith" in err and "conjunct" in err, err
    q = QueryPlan(small_table.col_types, aggs=[("sum", 0)]).to_spec()
    q.aggs[0].arith, q.aggs[0].col2 = R.DIV, 1
    h = eng.lib.bkgpu_filter_agg(small_table.handle, C.byref(q), 0, 64, 16)
    if h:
        eng.lib.bkgpu_agg_free(h)
    assert not h
    err = eng.lib.bkgpu_last_error().decode()
    assert "arith" in err and "aggregate" in err, err

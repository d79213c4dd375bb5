# Reference interpreter for the engine's postfix expression programs
# (include/bk_common.h BkExprOp): a small vectorized numpy evaluation of an
# op list exactly as plan.compile_expr emits it. It is the yardstick of
# tests/test_expr_cond_plan.py (checked there against hand-derived vectors,
# tests/golden/expr_cond_golden.json) and the per-row reference of
# tests/test_gpu_expr_cond.py. Semantics follow the reference's
# operators.cpp:18-103 and internal_functions.cpp:2351-2421; all operands
# are evaluated eagerly (ScalarFnCall::get_value), so a stack machine is
# exact.
import numpy as np

TYPE_INT64, TYPE_DOUBLE = 6, 12
(COL, LIT_I, LIT_D, ARITH, FN, NEG, CMP, IF, IFNULL, NULLIF, ISNULL,
 NULL) = range(12)
ADD, SUB, MUL, DIV, MOD = 1, 2, 3, 4, 5
EQ, NE, GT, GE, LT, LE = range(6)

# mnemonic op lists (the golden file's notation) -> op dicts
_ARITH_NAMES = {"add": ADD, "sub": SUB, "mul": MUL, "div": DIV, "mod": MOD}
_CMP_NAMES = {"eq": EQ, "ne": NE, "gt": GT, "ge": GE, "lt": LT, "le": LE}
_DOM = {"i": TYPE_INT64, "d": TYPE_DOUBLE}


def ops_from_mnemonics(mn):
    out = []
    for m in mn:
        t = m[0]
        if t == "col":
            out.append(dict(op=COL, arg=m[1]))
        elif t == "liti":
            out.append(dict(op=LIT_I, lit_i=int(m[1])))
        elif t == "litd":
            out.append(dict(op=LIT_D, lit_d=float(m[1])))
        elif t == "arith":
            out.append(dict(op=ARITH, arg=_ARITH_NAMES[m[1]],
                            domain=_DOM[m[2]]))
        elif t == "neg":
            out.append(dict(op=NEG, domain=_DOM[m[1]]))
        elif t == "cmp":
            out.append(dict(op=CMP, arg=_CMP_NAMES[m[1]], domain=_DOM[m[2]]))
        elif t == "if":
            out.append(dict(op=IF))
        elif t == "ifnull":
            out.append(dict(op=IFNULL))
        elif t == "nullif":
            out.append(dict(op=NULLIF, domain=_DOM[m[1]]))
        elif t == "isnull":
            out.append(dict(op=ISNULL))
        elif t == "null":
            out.append(dict(op=NULL))
        else:
            raise ValueError(f"bad mnemonic {m!r}")
    return out


def _i2d(i):
    return i.astype(np.float64)


def _d2i(d):
    # (int64_t)d truncates; out-of-range / non-finite has no defined int
    # view (never consumed: the planner reads a DOUBLE value's double view)
    ok = np.isfinite(d) & (np.abs(d) < 2.0 ** 63)
    return np.where(ok, d, 0.0).astype(np.int64)


def _scalar_fn(fn, v):
    # packed DATETIME fields (bk_common.h BK_DATETIME)
    u = v.astype(np.uint64)
    ym = (u >> np.uint64(46)) & np.uint64(0x1FFFF)
    out = {1: ym // np.uint64(13), 2: ym % np.uint64(13),
           3: (u >> np.uint64(41)) & np.uint64(31),
           4: (u >> np.uint64(36)) & np.uint64(31),
           5: (u >> np.uint64(30)) & np.uint64(63),
           6: (u >> np.uint64(24)) & np.uint64(63)}[fn]
    return out.astype(np.int64)


def eval_ops(ops, cols, valids):
    """ops: list of op dicts (op/arg/domain/lit_i/lit_d, missing = 0 with
    domain defaulting to INT64). cols: list of int64 / float64 arrays;
    valids: list of bool/uint8 arrays or None. Returns (valid, i, d):
    bool, int64 and float64 arrays — the stack slot's three views."""
    n = len(cols[0]) if cols else 1
    st = []
    with np.errstate(all="ignore"):
        for o in ops:
            op, arg = o.get("op", 0), o.get("arg", 0)
            dom = o.get("domain", TYPE_INT64)
            if op == COL:
                c = np.asarray(cols[arg])
                v = (np.ones(n, bool) if valids[arg] is None
                     else np.asarray(valids[arg]).astype(bool))
                if c.dtype == np.float64:
                    st.append((v, _d2i(c), c.copy()))
                else:
                    c = c.astype(np.int64)
                    st.append((v, c, _i2d(c)))
            elif op == LIT_I:
                i = np.full(n, int(o.get("lit_i", 0)), np.int64)
                st.append((np.ones(n, bool), i, _i2d(i)))
            elif op == LIT_D:
                d = np.full(n, float(o.get("lit_d", 0.0)), np.float64)
                st.append((np.ones(n, bool), _d2i(d), d))
            elif op == NULL:
                st.append((np.zeros(n, bool), np.zeros(n, np.int64),
                           np.zeros(n, np.float64)))
            elif op == ARITH:
                (vb, ib, db), (va, ia, da) = st.pop(), st.pop()
                v = va & vb
                if arg == DIV:
                    assert dom == TYPE_DOUBLE, "divide is DOUBLE-only"
                    v = v & (db != 0.0)          # -0.0 == 0.0: NULL too
                    d = da / np.where(v, db, 1.0)
                    st.append((v, _d2i(d), d))
                elif arg == MOD:
                    assert dom == TYPE_INT64, "mod is INT64-only"
                    v = v & (ib != 0)
                    # x % -1 == 0 == x % 1 (defines INT64_MIN % -1 as 0)
                    b = np.where(~v | (ib == -1), np.int64(1), ib)
                    i = np.fmod(ia, b)           # C %: sign of the dividend
                    st.append((v, i, _i2d(i)))
                elif dom == TYPE_DOUBLE:
                    d = {ADD: da + db, SUB: da - db, MUL: da * db}[arg]
                    st.append((v, _d2i(d), d))
                else:
                    ua, ub = ia.astype(np.uint64), ib.astype(np.uint64)
                    i = {ADD: ua + ub, SUB: ua - ub,
                         MUL: ua * ub}[arg].astype(np.int64)
                    st.append((v, i, _i2d(i)))
            elif op == FN:
                v, i, _ = st.pop()
                i = _scalar_fn(arg, i)
                st.append((v, i, _i2d(i)))
            elif op == NEG:
                v, i, d = st.pop()
                if dom == TYPE_DOUBLE:
                    d = -d
                    st.append((v, _d2i(d), d))
                else:
                    i = (np.uint64(0) - i.astype(np.uint64)).astype(np.int64)
                    st.append((v, i, _i2d(i)))
            elif op == CMP:
                (vb, ib, db), (va, ia, da) = st.pop(), st.pop()
                a, b = (da, db) if dom == TYPE_DOUBLE else (ia, ib)
                r = {EQ: a == b, NE: a != b, GT: a > b, GE: a >= b,
                     LT: a < b, LE: a <= b}[arg]
                i = r.astype(np.int64)
                st.append((va & vb, i, _i2d(i)))
            elif op == IF:
                e_, t_, c_ = st.pop(), st.pop(), st.pop()
                take = c_[0] & (c_[1] != 0)      # NULL condition -> else
                st.append(tuple(np.where(take, x, y)
                                for x, y in zip(t_, e_)))
            elif op == IFNULL:
                b_, a_ = st.pop(), st.pop()
                st.append(tuple(np.where(a_[0], x, y)
                                for x, y in zip(a_, b_)))
            elif op == NULLIF:
                (vb, ib, db), (va, ia, da) = st.pop(), st.pop()
                eq = (da == db) if dom == TYPE_DOUBLE else (ia == ib)
                st.append((va & ~(vb & eq), ia, da))
            elif op == ISNULL:
                v, _, _ = st.pop()
                i = (~v).astype(np.int64)
                st.append((np.ones(n, bool), i, _i2d(i)))
            else:
                raise ValueError(f"bad opcode {op}")
    assert len(st) == 1, "program must leave exactly one result"
    v, i, d = st[0]
    return v.astype(bool), i.astype(np.int64), d.astype(np.float64)


def eval_expr(expr, cols, valids):
    """Compile a plan.compile_expr tree and evaluate it; returns
    (domain, valid, value) with value in the expression's domain."""
    from baikaldb_amd.plan import compile_expr
    types = [TYPE_DOUBLE if np.asarray(c).dtype == np.float64 else TYPE_INT64
             for c in cols]
    ops = []
    dom = compile_expr(expr, types, ops)
    v, i, d = eval_ops(ops, cols, valids)
    return dom, v, (d if dom == TYPE_DOUBLE else i)

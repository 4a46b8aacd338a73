"""TEST HARNESS: `| GROUP BY ... YIELD ...` for the nGQL front end of tests/support/ngql.py, a
plain-Python model of GroupByExecutor (src/graph/GroupByExecutor.cpp:44-178 the checks, :226-322
the grouping, AggregateFunction.h the functions) as include/nbg.h restates it for nbg_group_by,
and a session that runs GO through any backend and GROUP BY through the model or through
``Engine.group_by`` on device-resident rows.

The model is the checker of tests/test_gpu_groupby.py; tests/test_groupby_model.py pins it to the
reference's own GroupByLimitTest vectors (tests/golden/groupby_golden.json) first.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass, field
from typing import List, Optional

from nebula_amd import _lib, expr as E
from nebula_amd.engine import NbgError
from tests.support import ngql

AGG_FUNS = ("COUNT", "COUNT_DISTINCT", "SUM", "AVG", "MAX", "MIN", "STD", "BIT_AND", "BIT_OR", "BIT_XOR")
STATUS = {_lib.OK: "SUCCEEDED", _lib.E_SYNTAX_ERROR: "E_SYNTAX_ERROR", _lib.E_EXECUTION_ERROR: "E_EXECUTION_ERROR",
          _lib.E_UNSUPPORTED: "E_UNSUPPORTED"}
# value types of an input column (common.thrift SupportedType names)
INT, VID, DOUBLE, BOOL, STRING, TIMESTAMP = "INT", "VID", "DOUBLE", "BOOL", "STRING", "TIMESTAMP"


class GroupError(Exception):
    """A GROUP BY the reference (or the device scope) answers with a status."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


@dataclass
class AggCol:
    fun: str            # "" for a plain column
    expr: E.Expr
    alias: Optional[str] = None

    def name(self):     # YieldColumn::toString
        if self.alias:
            return self.alias
        s = self.expr.to_string()
        return f"{self.fun}({s})" if self.fun else s


@dataclass
class GroupBySentence:
    groups: List[AggCol] = field(default_factory=list)
    yields: List[AggCol] = field(default_factory=list)


def split_pipes(text: str) -> List[str]:
    """The sentences of a statement: split at every top-level `|` (not `||`, not inside quotes or
    parentheses)."""
    out, cur, depth, quote, i = [], [], 0, None, 0
    while i < len(text):
        ch = text[i]
        if quote:
            cur.append(ch)
            if ch == "\\" and i + 1 < len(text):
                cur.append(text[i + 1])
                i += 1
            elif ch == quote:
                quote = None
        elif ch in "\"'":
            quote = ch
            cur.append(ch)
        elif ch == "|" and text[i + 1:i + 2] == "|":
            cur.append("||")
            i += 1
        elif ch == "|" and depth == 0:
            out.append("".join(cur))
            cur = []
        else:
            depth += (ch == "(") - (ch == ")")
            cur.append(ch)
        i += 1
    out.append("".join(cur))
    return out


class Parser(ngql.Parser):
    """ngql.Parser plus group_by_sentence (parser.yy:879-885) with yield_column's aggregate forms
    (:672-701): `FUN(expr)`, `FUN(*)` (the string primary "*") and `AS alias`."""

    def primary_sentence(self):
        if self.kw("GROUP"):
            return self.group_by()
        return super().primary_sentence()

    def group_by(self):
        self.expect_kw("GROUP")
        self.expect_kw("BY")
        g = GroupBySentence()
        g.groups = self.agg_cols()
        self.expect_kw("YIELD")
        g.yields = self.agg_cols()
        return g

    def agg_cols(self):
        cols = [self.agg_col()]
        while self.sym(","):
            self.take()
            cols.append(self.agg_col())
        return cols

    def agg_col(self):
        fun = ""
        if self.kw(*AGG_FUNS) and self.peek(1) == ("sym", "("):
            fun = self.take()[1].upper()
            self.take()
            if self.sym("*") and self.peek(1) == ("sym", ")"):
                self.take()
                e = E.const("*")
            else:
                e = self.expression()
            self.expect_sym(")")      # (a second argument is a syntax error, as in the grammar)
        else:
            e = self.expression()
        alias = None
        if self.kw("AS"):
            self.take()
            alias = self.take()[1]
        return AggCol(fun, e, alias)


def parse_sentence(text: str):
    p = Parser(text)
    s = p.primary_sentence()
    if p.peek()[0] != "eof":
        raise ngql.ParseError(f"trailing input near {p.peek()[1]!r}")
    return s


# ------------------------------------------------------------------------------------ the model
def type_of_value(v) -> str:
    if isinstance(v, bool):
        return BOOL
    if isinstance(v, float):
        return DOUBLE
    if isinstance(v, str):
        return STRING
    return INT


def _wrap(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= 1 << 63 else v


def fold(e: E.Expr):
    """A constant expression's value (the forms the device scope folds), else GroupError."""
    k = e.kind
    if k == E.K_PRIMARY:
        return e.value
    if k == E.K_UNARY:
        v = fold(e.args[0])
        if e.op == "!":
            return not v
        if isinstance(v, (bool, str)):
            raise GroupError(_lib.E_EXECUTION_ERROR, "bad operand")
        return -v if e.op == "-" else v
    if k == E.K_ARITH and e.op in "+-*":
        a, b = fold(e.args[0]), fold(e.args[1])
        if any(isinstance(x, (bool, str)) for x in (a, b)):
            raise GroupError(_lib.E_UNSUPPORTED, "model: arithmetic on non-numbers")
        r = a + b if e.op == "+" else a - b if e.op == "-" else a * b
        return _wrap(r) if isinstance(r, int) else r
    if k == E.K_FUNC and e.alias == "abs" and len(e.args) == 1:
        v = fold(e.args[0])
        return float(abs(v))     # FunctionManager abs returns a double
    raise GroupError(_lib.E_UNSUPPORTED, "neither `$-.col' nor a constant the model folds")


def _key_cell(v):
    return 0.0 if isinstance(v, float) and v == 0.0 else v


def aggregate(fun: str, vals: list, t: str):
    """One aggregate over a group's values of type `t` (nbg.h "Functions")."""
    n = len(vals)
    int_like = t in (INT, VID, TIMESTAMP)
    if fun == "":
        return vals[-1]
    if fun == "COUNT":
        return n
    if fun == "COUNT_DISTINCT":
        return len({(type(v).__name__, _key_cell(v)) for v in vals})
    if fun == "SUM":
        if int_like:
            return _wrap(sum(vals))
        if t == DOUBLE:
            s = vals[0]
            for v in vals[1:]:
                s += v
            return s
        return 0
    if fun == "AVG":
        if t in (VID, TIMESTAMP):
            raise GroupError(_lib.E_UNSUPPORTED, "AVG over a VID or TIMESTAMP column")
        if t == INT:
            return float(_wrap(sum(vals))) / n
        if t == DOUBLE:
            return aggregate("SUM", vals, t) / n
        return 0.0
    if fun in ("MAX", "MIN"):
        return max(vals) if fun == "MAX" else min(vals)
    if fun == "STD":
        if t not in (INT, DOUBLE):
            return 0
        avg = aggregate("AVG", vals, t)
        acc = 0.0
        for v in vals:
            x = float(v)
            acc += (x - avg) * (x - avg)
        return math.sqrt(acc / n)
    if t != INT:
        return 0
    r = vals[0]
    for v in vals[1:]:
        r = r & v if fun == "BIT_AND" else r | v if fun == "BIT_OR" else r ^ v
    return r


def group_model(inp: ngql.Interim, groups: List[AggCol], yields: List[AggCol], types=None) -> ngql.Interim:
    """GroupByExecutor over an Interim.  `types`: the input columns' types (default: from the first
    row's values, as the InterimResult schema is)."""
    names = [y.name() for y in yields]
    if not inp.rows:                       # execute() returns before checkAll
        return ngql.Interim(names, [])
    if types is None:
        types = [type_of_value(v) for v in inp.rows[0]]

    def syntax(msg):
        return GroupError(_lib.E_SYNTAX_ERROR, msg)
    # prepareYield / prepareGroup
    if not yields:
        raise syntax("Yield cols is empty")
    aliases = {}
    for y in yields:
        if y.fun not in ("COUNT", "COUNT_DISTINCT") and y.expr.kind == E.K_PRIMARY and y.expr.value == "*" \
                and isinstance(y.expr.value, str):
            raise syntax("Syntax error: near `*'")
        if y.alias and y.expr.kind == E.K_INPUT:
            aliases.setdefault(y.alias, y)
    if not groups:
        raise syntax("Group cols is empty")
    for g in groups:
        if g.fun:
            raise syntax(f"Use invalid group function `{g.fun}'")
    # checkAll
    keys, key_set = [], set()
    for g in groups:
        e = g.expr
        if e.kind == E.K_INPUT:
            if e.prop not in inp.columns:
                raise syntax(f"Group `{e.prop}' isn't in output fields")
        elif e.kind == E.K_FUNC:
            continue
        else:
            name = e.to_string()
            if name not in aliases:
                raise syntax(f"Group `{name}' isn't in output fields")
            e = aliases[name].expr
        key_set.add(e.prop)
        if e.prop in inp.columns and inp.columns.index(e.prop) not in keys:
            keys.append(inp.columns.index(e.prop))
    for y in yields:
        if y.expr.kind == E.K_INPUT:
            if y.expr.prop not in inp.columns:
                raise syntax(f"Yield `{y.expr.prop}' isn't in output fields")
            if not y.fun and y.expr.prop not in key_set:
                raise syntax(f"Yield `{y.expr.prop}' isn't in group fields")
        elif y.expr.kind == E.K_VAR:
            raise syntax("Can't support variableExpression")
    for g in groups:
        if g.expr.kind == E.K_FUNC:
            fold(g.expr)
    # groupingData
    operands = []
    for y in yields:
        if y.expr.kind == E.K_INPUT:
            c = inp.columns.index(y.expr.prop)
            operands.append((c, None, types[c]))
        else:
            v = 1 if (y.expr.kind == E.K_PRIMARY and y.expr.value == "*") else fold(y.expr)
            operands.append((None, v, type_of_value(v)))
    data = {}
    for r in inp.rows:
        data.setdefault(tuple((type(r[c]).__name__, _key_cell(r[c])) for c in keys), []).append(r)
    rows = []
    for members in data.values():
        row = []
        for y, (c, const, t) in zip(yields, operands):
            vals = [m[c] for m in members] if c is not None else [const] * len(members)
            row.append(aggregate(y.fun, vals, t))
        rows.append(row)
    return ngql.Interim(names, rows)


# ------------------------------------------------------------------------------------ execution
def go_column_types(g: ngql.GoSentence, rows):
    """Types of a GO result's columns as far as GROUP BY tells them apart: `_dst` / `_src` columns
    are VIDs, everything else follows the first row's values."""
    if not rows:
        return None
    out = [type_of_value(v) for v in rows[0]]
    for i, y in enumerate(g.yields or []):
        if y.expr.kind in (E.K_DST, E.K_SRCID) and i < len(out):
            out[i] = VID
    if g.yields is None:
        out = [VID] * len(out)
    return out


class Session(ngql.Session):
    """ngql.Session plus GROUP BY.  GO runs on `backend`; GROUP BY runs through the model, or —
    with `device=True` on an Engine backend — through Engine.group_by over the rows the GO in
    front of it left on the device (go_device -> group_by -> fetch)."""

    def __init__(self, backend, device=False):
        super().__init__(backend)
        self.device = device
        self.last_types = None

    def execute(self, text: str) -> ngql.Interim:
        result = None
        parts = split_pipes(text)
        i = 0
        while i < len(parts):
            st = parse_sentence(parts[i])
            nxt = parse_sentence(parts[i + 1]) if i + 1 < len(parts) else None
            if self.device and isinstance(st, ngql.GoSentence) and isinstance(nxt, GroupBySentence):
                result = self._go_group_device(st, nxt, result)
                i += 2
                continue
            result = self._run(st, result)
            i += 1
        return result

    def status(self, text: str):
        """(status name, result or None): what a client sees."""
        try:
            return "SUCCEEDED", self.execute(text)
        except ngql.ParseError:
            return "E_SYNTAX_ERROR", None
        except GroupError as ex:
            return STATUS.get(ex.code, str(ex.code)), None
        except NbgError as ex:
            return STATUS.get(ex.code, str(ex.code)), None

    def _run(self, st, inp):
        if isinstance(st, GroupBySentence):
            if inp is None:
                return ngql.Interim([y.name() for y in st.yields], [])
            return group_model(inp, st.groups, st.yields, self.last_types)
        r = super()._run(st, inp)
        self.last_types = go_column_types(st, r.rows) if isinstance(st, ngql.GoSentence) else None
        return r

    def _go_group_device(self, g: ngql.GoSentence, gb: GroupBySentence, inp):
        if g.upto or g.reversely or g.over_all or g.yields is None:
            raise ngql.ExecError("device GROUP BY harness: GO needs OVER names and a YIELD")
        etypes = self._edge_types(g.over, False)
        names = [c.name() for c in g.yields]
        if g.from_ref is not None:
            src = self._source(g.from_ref, inp)
            starts = [int(v) for v in src.col(g.from_ref[1])] if src is not None and src.rows else []
        else:
            starts = list(g.from_vids)
        rows = self.b.go_device(starts, etypes, g.steps, g.where.encode() if g.where else b"",
                                [c.expr.encode() for c in g.yields], g.distinct)
        try:
            # (the request has no function field for group columns: a call named like the aggregate)
            out = self.b.group_by(rows, names,
                                  [(E.Expr(E.K_FUNC, alias=c.fun, args=[c.expr]) if c.fun else c.expr).encode()
                                   for c in gb.groups],
                                  [(c.fun, c.expr.encode(), c.alias) for c in gb.yields])
        finally:
            rows.free()
        try:
            return ngql.Interim([c.name() for c in gb.yields], out.fetch())
        finally:
            out.free()


# ------------------------------------------------------------------------------------ comparing
def cell(v):
    """A result cell with its kind, -0.0 folded into 0.0 (which sign a key reports is unspecified)."""
    if isinstance(v, float):
        return ("double", struct.pack("<d", v + 0.0 if v != 0.0 else 0.0))
    return (type(v).__name__, v)


def multiset(rows):
    return sorted((tuple(cell(v) for v in r) for r in rows), key=repr)


def run_case(session: Session, case):
    """(ok, message) for one groupby_golden.json case: status, column names where the reference's
    test asserts them, and the rows as a multiset with their kinds."""
    st, res = session.status(case["query"])
    if st != case["status"]:
        return False, f"status {st} != {case['status']}"
    if st != "SUCCEEDED":
        return True, "failed as expected"
    if "col_names" in case and res.columns != case["col_names"]:
        return False, f"columns {res.columns} != {case['col_names']}"
    got, exp = multiset(res.rows), multiset(case["expected"])
    return got == exp, "" if got == exp else f"rows {res.rows} != {case['expected']}"

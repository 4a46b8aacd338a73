"""TEST HARNESS: `UNION [ALL|DISTINCT]`, `INTERSECT` and `MINUS` for the nGQL front end of
tests/support/ngql.py, groupby.py and orderby.py, a plain-Python model of SetExecutor
(src/graph/SetExecutor.cpp:98-383) as include/nbg.h restates it for nbg_set_op, and a session whose
device mode keeps the operands and the set operations in HBM.

The model is the checker of tests/test_gpu_setops.py and tests/test_gpu_values_setops.py;
tests/test_setops_model.py pins it to the reference's own SetTest vectors
(tests/golden/setop_golden.json) first.

Grammar (parser.yy:1095-1141): a set_sentence is piped sentences joined by the three operators,
which share one priority and associate to the left; `( set_sentence )` and `( piped_sentence )` are
sentences themselves.  A set sentence as the right side of a pipe is a syntax error
(PipeExecutor::prepare, "Set op not support input.").
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass
from typing import Optional

from nebula_amd import _lib, expr as E
from nebula_amd.engine import NbgError
from tests.support import groupby, ngql, orderby
from tests.support.groupby import BOOL, DOUBLE, INT, STRING, TIMESTAMP, VID, GroupError
from tests.support.oracle import OracleError

UNION, INTERSECT, MINUS = "UNION", "INTERSECT", "MINUS"
INT_LIKE = (INT, VID, TIMESTAMP)


# ------------------------------------------------------------------------------------ parsing
@dataclass
class SetNode:
    left: object
    op: str
    distinct: bool        # UNION only
    right: object


@dataclass
class PipeNode:
    parts: list           # sentence texts and, for `( ... )`, the SetNode / PipeNode inside


def _top_level(text: str):
    """(index, char, depth 0 and outside quotes) for every character."""
    depth, quote, i = 0, None, 0
    while i < len(text):
        ch = text[i]
        if quote:
            if ch == "\\":
                i += 1
            elif ch == quote:
                quote = None
            yield i, ch, False
        elif ch in "\"'":
            quote = ch
            yield i, ch, False
        else:
            if ch == ")":
                depth -= 1
            yield i, ch, depth == 0
            if ch == "(":
                depth += 1
        i += 1


def _split_set(text: str):
    """[operand, (op, distinct), operand, ...] of a set_sentence's text."""
    out, start, i = [], 0, 0
    top = {i: t for i, _, t in _top_level(text)}
    while i < len(text):
        if top.get(i) and (i == 0 or not (text[i - 1].isalnum() or text[i - 1] in "_$.")):
            for word in (UNION, INTERSECT, MINUS):
                end = i + len(word)
                if text[i:end].upper() == word and (end == len(text) or not (text[end].isalnum() or text[end] == "_")):
                    out.append(text[start:i])
                    distinct = False
                    if word == UNION:
                        rest = text[end:].lstrip()
                        skipped = len(text[end:]) - len(rest)
                        distinct = True
                        for mod in ("ALL", "DISTINCT"):
                            if rest[:len(mod)].upper() == mod and not (rest[len(mod):len(mod) + 1].isalnum()):
                                distinct = mod == "DISTINCT"
                                end += skipped + len(mod)
                    out.append((word, distinct))
                    start = i = end
                    break
            else:
                i += 1
            continue
        i += 1
    out.append(text[start:])
    return out


def parse_statement(text: str):
    """The SetNode / PipeNode tree of one statement."""
    items = _split_set(text)
    node = _parse_piped(items[0])
    for k in range(1, len(items), 2):
        op, distinct = items[k]
        node = SetNode(node, op, distinct, _parse_piped(items[k + 1]))
    return node


def _parse_piped(text: str) -> PipeNode:
    if not text.strip():
        raise ngql.ParseError("a set operator needs a sentence on both sides")
    parts = []
    for k, p in enumerate(groupby.split_pipes(text)):
        p = p.strip()
        if p.startswith("("):
            if not p.endswith(")") or any(top and i < len(p) - 1 for i, _, top in _top_level(p) if i > 0):
                raise ngql.ParseError(f"unbalanced parentheses near {p[:20]!r}")
            inner = parse_statement(p[1:-1])
            if k > 0 and isinstance(inner, SetNode):
                raise ngql.ParseError("Set op not support input.")
            parts.append(inner)
        else:
            orderby.parse_sentence(p)          # (syntax errors surface before anything runs)
            parts.append(p)
    return PipeNode(parts)


# ------------------------------------------------------------------------------------ the model
def cast_value(v, from_t: str, to_t: str):
    """InterimResult::castTo* (InterimResult.cpp:292-538) for one right-side cell."""
    if from_t == to_t or (from_t in INT_LIKE and to_t in INT_LIKE):
        return v
    if to_t in INT_LIKE:
        if from_t == DOUBLE:
            if math.isnan(v) or abs(v) >= 2.0 ** 63:
                raise GroupError(_lib.E_UNSUPPORTED, "model: the reference's cast of this double is undefined")
            return math.trunc(v)
        if from_t == BOOL:
            return int(v)
    if to_t == DOUBLE:
        if from_t in INT_LIKE:
            return float(v)                    # (int -> float rounds to nearest even, as (double) does)
        if from_t == BOOL:
            return 1.0 if v else 0.0
    if to_t == BOOL:
        if from_t in INT_LIKE:
            return v != 0
        if from_t == DOUBLE:
            return v != 0.0                    # (NaN != 0.0 is true, -0.0 != 0.0 is false)
    if to_t == STRING and from_t in INT_LIKE:
        return str(v)                          # folly::to<std::string>(int64_t)
    raise GroupError(_lib.E_UNSUPPORTED, f"model: cast {from_t} -> {to_t}")


def _bits(v: float) -> int:
    return struct.unpack("<q", struct.pack("<d", v))[0]


def row_key(row, by_bits=False):
    """What two equal rows share: IEEE == for doubles (-0.0 is 0.0); `by_bits` keeps NaNs apart by
    their bits (UNION DISTINCT).  None for a row holding a NaN otherwise: it equals nothing."""
    key = []
    for v in row:
        if isinstance(v, float):
            if math.isnan(v):
                if not by_bits:
                    return None
                key.append(("nan", _bits(v)))
            else:
                key.append(("double", 0.0 if v == 0.0 else v))
        else:
            key.append((type(v).__name__, v))
    return tuple(key)


def column_types(inp: ngql.Interim, types=None):
    if types is not None:
        return list(types)
    return [groupby.type_of_value(v) for v in inp.rows[0]] if inp.rows else [INT] * len(inp.columns)


def set_model(left: ngql.Interim, right: ngql.Interim, op: str, distinct=False, ltypes=None, rtypes=None):
    """SetExecutor over two Interims -> (Interim, column types).  The result has the left's column
    names; UNION ALL is the left's rows followed by the right's, the other orders are arbitrary."""
    if len(left.columns) != len(right.columns):
        raise GroupError(_lib.E_EXECUTION_ERROR, "Field count not match.")
    lt, rt = column_types(left, ltypes), column_types(right, rtypes)
    # the empty-input shortcuts, before any schema check
    if not left.rows or not right.rows:
        if op == UNION and right.rows:
            return ngql.Interim(left.columns, [list(r) for r in right.rows]), rt
        if op in (UNION, MINUS) and left.rows:
            return ngql.Interim(left.columns, [list(r) for r in left.rows]), lt
        return ngql.Interim(left.columns, []), lt
    cast = [[cast_value(v, f, t) for v, f, t in zip(r, rt, lt)] for r in right.rows]
    lrows = [list(r) for r in left.rows]
    if op == UNION:
        rows = lrows + cast
        if distinct:
            seen = {}
            for r in rows:
                seen.setdefault(row_key(r, by_bits=True), r)
            rows = list(seen.values())
    elif op == INTERSECT:                      # every right row is used up by one left row
        have = {}
        for r in cast:
            k = row_key(r)
            if k is not None:
                have[k] = have.get(k, 0) + 1
        rows = []
        for r in lrows:
            k = row_key(r)
            if k is not None and have.get(k, 0) > 0:
                have[k] -= 1
                rows.append(r)
    elif op == MINUS:
        have = {row_key(r) for r in cast} - {None}
        rows = [r for r in lrows if row_key(r) not in have]
    else:
        raise GroupError(_lib.E_INVALID_ARGUMENT, "unknown operator")
    return ngql.Interim(left.columns, rows), lt


# ------------------------------------------------------------------------------------ execution
class Value:
    """An operand or result: its column names and types and either device rows or an Interim."""

    def __init__(self, names, types=None, rows=None, interim=None):
        self.names, self.types, self.rows, self.interim = list(names), types, rows, interim

    def fetch(self) -> ngql.Interim:
        if self.interim is None:
            self.interim = ngql.Interim(self.names, self.rows.fetch())
        return self.interim

    def free(self):
        if self.rows is not None:
            self.rows.free()
            self.rows = None


class Session(orderby.Session):
    """orderby.Session plus the set operators.  Without `device` everything after the GOs runs in
    the models.  With it, each operand's last GO runs with go_device (with the GROUP BY / ORDER BY /
    LIMIT stages behind it, as orderby.Session does), every set operation is Engine.set_op over
    device rows, and the statement fetches once at its end — or where a following `| GO FROM $-.x`
    needs its input on the host.  An operand that is itself a pipe runs its earlier sentences the
    way orderby.Session does.  A set_op the engine answers with NBG_E_UNSUPPORTED falls back to
    the model over the fetched operands and is recorded in `fallbacks`; `set_calls` lists the
    operators nbg_set_op completed."""

    def __init__(self, backend, device=False):
        super().__init__(backend, device)
        self.set_calls, self.fallbacks = [], []

    def execute(self, text: str) -> ngql.Interim:
        self.set_calls, self.fallbacks = [], []
        v = self._eval(parse_statement(text), None)
        try:
            return v.fetch()
        finally:
            v.free()

    # -- operands
    def _operand_error(self, ex):
        """SetExecutor::execute wraps an operand's failure: `lhs has error: ... rhs has error: ...`."""
        code = getattr(ex, "code", _lib.E_EXECUTION_ERROR)
        if code == _lib.E_SYNTAX_ERROR:
            return ex
        return GroupError(_lib.E_EXECUTION_ERROR, f"lhs has error: / rhs has error: {ex}")

    def _eval(self, node, inp: Optional[ngql.Interim]) -> Value:
        if isinstance(node, SetNode):
            try:
                lv = self._eval(node.left, None)
            except (GroupError, NbgError, OracleError, ngql.ExecError) as ex:
                raise self._operand_error(ex)
            try:
                rv = self._eval(node.right, None)
            except (GroupError, NbgError, OracleError, ngql.ExecError) as ex:
                lv.free()
                raise self._operand_error(ex)
            try:
                return self._set(lv, rv, node.op, node.distinct)
            finally:
                lv.free()
                rv.free()
        return self._pipe(node.parts, inp)

    def _pipe(self, parts, inp) -> Value:
        """A piped sentence: runs of plain sentences go through orderby.Session's own loop; in
        device mode the last run ends on the device when it is `GO [| stages]`."""
        val = Value(inp.columns, interim=inp) if inp is not None else None
        i = 0
        while i < len(parts):
            if not isinstance(parts[i], str):
                nxt = self._eval(parts[i], val.fetch() if val is not None else None)
                if val is not None:
                    val.free()
                val = nxt
                i += 1
                continue
            j = i
            while j < len(parts) and isinstance(parts[j], str):
                j += 1
            cur = val.fetch() if val is not None else None
            if val is not None:
                val.free()
            val = self._sentences([orderby.parse_sentence(p) for p in parts[i:j]], cur, last=j == len(parts))
            i = j
        return val

    def _sentences(self, sents, result, last) -> Value:
        for st in sents:                  # every executor's prepare() runs before the first execute()
            if isinstance(st, orderby.LimitSentence):
                orderby.check_limit(st.offset, st.count)
        tail = None                       # the `GO [| stages]` that can stay on the device
        if self.device and last:
            g = len(sents) - 1
            while g >= 0 and isinstance(sents[g], orderby.STAGES):
                g -= 1
            if g >= 0 and isinstance(sents[g], ngql.GoSentence) and self._device_go(sents[g]):
                tail, sents = sents[g:], sents[:g]
        i = 0
        while i < len(sents):
            st = sents[i]
            if self.device and isinstance(st, ngql.GoSentence) and i + 1 < len(sents) and isinstance(sents[i + 1], orderby.STAGES):
                j = i + 1
                while j < len(sents) and isinstance(sents[j], orderby.STAGES):
                    j += 1
                result = self._go_stages_device(st, sents[i + 1:j], result)
                self.last_types = None
                i = j
                continue
            result = self._run(st, result)
            i += 1
        if tail is None:
            if result is None:
                result = ngql.Interim([], [])
            return Value(result.columns, self.last_types, interim=result)
        return self._go_stages_rows(tail[0], tail[1:], result)

    @staticmethod
    def _device_go(g: ngql.GoSentence):
        """go_device takes no $- / $var rows: a GO reading input props runs through the host."""
        if g.upto or g.reversely or g.over_all or g.yields is None:
            return False
        cols = list(g.yields) + ([ngql.YieldCol(g.where)] if g.where else [])
        return not any(n.kind in (E.K_INPUT, E.K_VAR) for c in cols for n in c.expr.walk())

    def _go_stages_rows(self, g: ngql.GoSentence, stages, inp) -> Value:
        """orderby.Session._go_stages_device without its fetch."""
        etypes = self._edge_types(g.over, False)
        names = [c.name() for c in g.yields]
        if g.from_ref is not None:
            src = self._source(g.from_ref, inp)
            starts = [int(v) for v in src.col(g.from_ref[1])] if src is not None and src.rows else []
        else:
            starts = list(g.from_vids)
        rows = self.b.go_device(starts, etypes, g.steps, g.where.encode() if g.where else b"",
                                [c.expr.encode() for c in g.yields], g.distinct)
        types = self._go_types(g)
        try:
            k = 0
            while k < len(stages):
                st = stages[k]
                if isinstance(st, groupby.GroupBySentence):
                    nxt = self.b.group_by(rows, names,
                                          [(E.Expr(E.K_FUNC, alias=c.fun, args=[c.expr]) if c.fun else c.expr).encode()
                                           for c in st.groups],
                                          [(c.fun, c.expr.encode(), c.alias) for c in st.yields])
                    names = [c.name() for c in st.yields]
                    types = None
                else:
                    factors, limit = [], None
                    if isinstance(st, orderby.OrderBySentence):
                        factors = st.factors
                        if k + 1 < len(stages) and isinstance(stages[k + 1], orderby.LimitSentence):
                            k += 1
                            limit = (stages[k].offset, stages[k].count)
                    else:
                        limit = (st.offset, st.count)
                    nxt = self.b.order_by(rows, names, factors, limit)
                k += 1
                rows.free()
                rows = nxt
        except Exception:
            rows.free()
            raise
        return Value(names, types, rows=rows)

    @staticmethod
    def _go_types(g: ngql.GoSentence):
        """VID for `_dst` / `_src` columns, None (from the values) for the others."""
        return [VID if y.expr.kind in (E.K_DST, E.K_SRCID) else None for y in g.yields]

    # -- the operators
    @staticmethod
    def _types(v: Value, inp: ngql.Interim):
        by_value = column_types(inp)
        if v.types is None:
            return by_value
        return [t if t is not None else b for t, b in zip(v.types, by_value)]

    def _set(self, lv: Value, rv: Value, op: str, distinct: bool) -> Value:
        if self.device and lv.rows is not None and rv.rows is not None:
            try:
                out = self.b.set_op(lv.rows, rv.rows, op, distinct)
            except NbgError as ex:
                if ex.code != _lib.E_UNSUPPORTED:
                    raise
                self.fallbacks.append((op, ex.code))
            else:
                self.set_calls.append((op, distinct))
                # (a passed-on right side keeps its own types: only the shortcut for an empty left)
                types = rv.types if op == UNION and not lv.rows.count and rv.rows.count else lv.types
                return Value(lv.names, types, rows=out)
        li, ri = lv.fetch(), rv.fetch()
        res, types = set_model(li, ri, op, distinct, self._types(lv, li), self._types(rv, ri))
        return Value(lv.names, types, interim=res)


# ------------------------------------------------------------------------------------ comparing
def bits_cell(v):
    """A result cell with its kind; doubles by their bits (NaN payloads and zero signs kept)."""
    if isinstance(v, float):
        return ("double", _bits(v))
    return (type(v).__name__, v)


def run_case(session: Session, case):
    """(ok, message) for one setop_golden.json case: status, column names where the reference's
    test asserts them, `no_rows`, and the rows as a multiset with their kinds."""
    st, res = session.status(case["query"])
    if st != case["status"]:
        return False, f"status {st} != {case['status']}"
    if st != "SUCCEEDED":
        return True, "failed as expected"
    if "col_names" in case and res.columns != case["col_names"]:
        return False, f"columns {res.columns} != {case['col_names']}"
    if case.get("no_rows") and res.rows:
        return False, f"{len(res.rows)} rows where the reference has none"
    if "expected" not in case:
        return True, ""
    got, exp = groupby.multiset(res.rows), groupby.multiset(case["expected"])
    return got == exp, "" if got == exp else f"rows {res.rows} != {case['expected']}"

"""TEST HARNESS: the piped `YIELD cols [WHERE expr]` sentence for the nGQL front end of
tests/support/ngql.py, groupby.py, orderby.py and setops.py, a plain-Python model of YieldExecutor
(src/graph/YieldExecutor.cpp:178-282) as include/nbg.h restates it for nbg_yield, and a session
whose device mode keeps the YIELD stage in HBM beside GROUP BY / ORDER BY / LIMIT and the set
operators.

The model is the checker of tests/test_gpu_yield.py and tests/test_gpu_values_yield.py;
tests/test_yield_model.py pins it to the reference's own YieldTest vectors
(tests/golden/yield_golden.json) and its evaluator to tests/golden/expression_cases.json first.

Grammar (parser.yy:707-713): `YIELD yield_columns [WHERE expression]`; a YIELD sentence has no
DISTINCT.  It stands alone (`$var = GO ...; YIELD $var.x`), as a pipe stage, and inside the
operands of the set operators.

The evaluator covers a stated subset of Expressions.cpp, enough for arithmetic, comparisons and
casts over columns: wrapping int64 `+ - * / %` (division by zero and INT64_MIN / -1 are evaluation
errors), `^` on ints, IEEE double arithmetic, the 1e-8 double equality, `<`-derived relations
(`a <= b` is `!(b < a)`, so a NaN makes <= and >= true), `&& || XOR !` over asBool of numbers and
bools, unary minus, casts among int / timestamp / double / bool, hash of an int or a string, and
string compares by bytes.  Anything else raises ModelScope.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional

from nebula_amd import _lib, expr as E
from nebula_amd.engine import NbgError
from nebula_amd.vidhash import std_hash
from tests.support import groupby, ngql, orderby, setops
from tests.support.groupby import BOOL, DOUBLE, INT, STRING, TIMESTAMP, AggCol, GroupBySentence, GroupError
from tests.support.orderby import LimitSentence, OrderBySentence
from tests.support.setops import PipeNode, SetNode, Value

INT64_MIN = -(1 << 63)
GRAPH_KINDS = (E.K_SRC, E.K_DESTP, E.K_ALIAS, E.K_RANK, E.K_DST, E.K_SRCID, E.K_TYPE)
CAST_TYPES = {"int": INT, "bigint": INT, "timestamp": TIMESTAMP, "double": DOUBLE, "bool": BOOL, "string": STRING}


# ------------------------------------------------------------------------------------ parsing
@dataclass
class YieldSentence:
    yields: List[AggCol] = field(default_factory=list)
    where: Optional[E.Expr] = None

    def nodes(self):
        for c in self.yields:
            yield from c.expr.walk()
        if self.where is not None:
            yield from self.where.walk()

    def variables(self):
        """The variable names referenced, in order of appearance, without repeats."""
        return list(dict.fromkeys(n.alias for n in self.nodes() if n.kind == E.K_VAR))

    def uses_input(self):
        return any(n.kind == E.K_INPUT for n in self.nodes())

    def is_constant(self):
        """Neither `$-' nor `$var': YieldExecutor::executeConstant, one row."""
        return not self.uses_input() and not self.variables()


STAGES = (GroupBySentence, OrderBySentence, LimitSentence, YieldSentence)


class Parser(orderby.Parser):
    """orderby.Parser plus yield_sentence, with yield_column's aggregate forms (groupby.Parser)."""

    def primary_sentence(self):
        if self.kw("YIELD"):
            return self.yield_sentence()
        return super().primary_sentence()

    def yield_sentence(self):
        self.expect_kw("YIELD")
        s = YieldSentence(self.agg_cols())
        if self.kw("WHERE"):
            self.take()
            s.where = self.expression()
        return s


def parse_sentence(text: str):
    p = Parser(text)
    s = p.primary_sentence()
    if p.peek()[0] != "eof":
        raise ngql.ParseError(f"trailing input near {p.peek()[1]!r}")
    return s


def split_statements(text: str):
    """[(variable or None, statement text)] of `stmt; $v = stmt; ...` (top-level semicolons)."""
    parts, start = [], 0
    for i, ch, top in setops._top_level(text):
        if ch == ";" and top:
            parts.append(text[start:i])
            start = i + 1
    parts.append(text[start:])
    out = []
    for p in parts:
        p = p.strip()
        if not p:
            continue
        var = None
        toks = ngql.tokenize(p)
        if toks[0][0] == "var" and toks[1] == ("sym", "="):
            var = toks[0][1][1:]
            p = p[p.index("=") + 1:]
        out.append((var, p))
    return out


def parse_statement(text: str):
    """setops.parse_statement with the YIELD sentence: the SetNode / PipeNode tree."""
    items = setops._split_set(text)
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
            if not p.endswith(")") or any(top and i < len(p) - 1 for i, _, top in setops._top_level(p) if i > 0):
                raise ngql.ParseError(f"unbalanced parentheses near {p[:20]!r}")
            inner = parse_statement(p[1:-1])
            if k > 0 and isinstance(inner, SetNode):
                raise ngql.ParseError("Set op not support input.")
            parts.append(inner)
        else:
            parse_sentence(p)                  # (syntax errors surface before anything runs)
            parts.append(p)
    return PipeNode(parts)


# ------------------------------------------------------------------------------------ the evaluator
class EvalError(Exception):
    """An evaluation error of the reference (a failed OptVariantType)."""


class ModelScope(Exception):
    """Outside the evaluator's stated subset."""


def _wrap(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= 1 << 63 else v


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _is_arith(v):
    return _is_int(v) or isinstance(v, float)


def as_bool(v):
    """Expression::asBool over numbers and bools."""
    if isinstance(v, bool):
        return v
    if _is_int(v):
        return v != 0
    if isinstance(v, float):
        return v != 0.0
    raise ModelScope("asBool of a string")


def _fdiv(a: float, b: float) -> float:
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _fmod(a: float, b: float) -> float:
    try:
        return math.fmod(a, b)
    except ValueError:
        return math.nan


def _to_double(v):
    if isinstance(v, bool):
        return 1.0 if v else 0.0
    return float(v)


def cast(ctype: str, v):
    """TypeCastingExpression::eval (Expressions.cpp:773-793) among int / timestamp / double / bool."""
    if ctype == "bigint":
        raise EvalError("Type bigint not supported yet")
    if ctype == "string" or isinstance(v, str):
        raise ModelScope("a cast to or from a string")
    if ctype in ("int", "timestamp"):
        if isinstance(v, float):
            if v != v or abs(v) >= 2.0 ** 63:
                raise ModelScope("(int) of a NaN or of a double beyond int64 is undefined in the reference")
            return math.trunc(v)
        return int(v)
    if ctype == "double":
        return _to_double(v)
    if ctype == "bool":
        return as_bool(v)
    raise ModelScope("cast " + ctype)


def evaluate(e: E.Expr, get=None):
    """The value of `e`; get(node) reads a `$-.x' / `$var.x' node.  Both operands of a binary node
    are evaluated (no short circuit) and the left one's error wins, as in the reference."""
    k = e.kind
    if k == E.K_PRIMARY:
        return e.value
    if k in (E.K_INPUT, E.K_VAR):
        if get is None:
            raise EvalError("no input")
        return get(e)
    if k == E.K_UNARY:
        v = evaluate(e.args[0], get)
        if e.op == "+":
            return v
        if e.op == "-":
            if _is_int(v):
                return _wrap(-v)
            if isinstance(v, float):
                return -v
            raise EvalError("attempt to perform unary arithmetic")
        return not as_bool(v)
    if k == E.K_CAST:
        return cast(e.op, evaluate(e.args[0], get))
    if k == E.K_FUNC:
        if e.alias.lower() == "hash" and len(e.args) == 1:
            v = evaluate(e.args[0], get)
            if _is_int(v):
                return v                      # std::hash<int64_t> is the identity
            if isinstance(v, str):
                return std_hash(v)
        raise ModelScope("function " + e.alias)
    if k not in (E.K_ARITH, E.K_REL, E.K_LOGIC):
        raise ModelScope(f"expression kind {k}")
    errs, vals = [], []
    for a in e.args:
        try:
            vals.append(evaluate(a, get))
        except EvalError as ex:
            errs.append(ex)
            vals.append(None)
    if errs:
        raise errs[0]
    l, r = vals
    if k == E.K_LOGIC:
        a, b = as_bool(l), as_bool(r)
        return (a and b) if e.op == "&&" else (a or b) if e.op == "||" else a != b
    if k == E.K_ARITH:
        if not (_is_arith(l) and _is_arith(r)):
            if e.op == "+" and isinstance(l, str) and isinstance(r, str):
                raise ModelScope("string concatenation")
            raise EvalError("attempt to perform arithmetic on a non-number")
        if isinstance(l, float) or isinstance(r, float):
            a, b = float(l), float(r)
            if e.op == "+":
                return a + b
            if e.op == "-":
                return a - b
            if e.op == "*":
                return a * b
            if e.op == "/":
                return _fdiv(a, b)
            if e.op == "%":
                return _fmod(a, b)
            raise ModelScope("^ over doubles")
        if e.op == "+":
            return _wrap(l + r)
        if e.op == "-":
            return _wrap(l - r)
        if e.op == "*":
            return _wrap(l * r)
        if e.op == "^":
            return l ^ r
        if r == 0 or (l == INT64_MIN and r == -1):
            raise EvalError("integer division by zero or overflow")
        q = abs(l) // abs(r)                   # C++ truncates toward zero
        q = -q if (l < 0) != (r < 0) else q
        return q if e.op == "/" else l - q * r
    # relational: implicitCasting bool -> int64 -> double (Expressions.cpp:1027-1045)
    def cls(v):
        return "b" if isinstance(v, bool) else "i" if isinstance(v, int) else "d" if isinstance(v, float) else "s"
    if cls(l) != cls(r):
        if "s" in (cls(l), cls(r)):
            raise EvalError("A string type can not be compared with a non-string type.")
        if "d" in (cls(l), cls(r)):
            l, r = _to_double(l), _to_double(r)
        else:
            l, r = int(l), int(r)
    if isinstance(l, str):
        l, r = l.encode(), r.encode()

    def lt(a, b):
        return a < b
    if e.op == "<":
        return lt(l, r)
    if e.op == "<=":
        return not lt(r, l)
    if e.op == ">":
        return lt(r, l)
    if e.op == ">=":
        return not lt(l, r)
    eq = abs(l - r) < 1e-8 if isinstance(l, float) else l == r
    return eq if e.op == "==" else not eq


# ------------------------------------------------------------------------------------ the model
def yield_checks(st: YieldSentence):
    """nbg.h statuses 3 and 4: checkAggFun and syntaxCheck."""
    if any(c.fun for c in st.yields):
        for c in st.yields:
            if c.expr.kind in (E.K_INPUT, E.K_VAR) and not c.fun:
                raise GroupError(_lib.E_SYNTAX_ERROR, "Input columns without aggregation are not supported in YIELD "
                                 f"statement without GROUP BY, near `{c.expr.to_string()}'")
    if any(n.kind in GRAPH_KINDS for n in st.nodes()):
        raise GroupError(_lib.E_SYNTAX_ERROR, "Only support input and variable in yield sentence.")
    if st.uses_input() and st.variables():
        raise GroupError(_lib.E_EXECUTION_ERROR, "Not support both input and variable.")
    if len(st.variables()) > 1:
        raise GroupError(_lib.E_EXECUTION_ERROR, "Only one variable allowed to use.")


def expand(yields: List[AggCol], columns) -> List[AggCol]:
    """YieldClauseWrapper::prepare: `$-.*' / `$var.*' is every input column, in order."""
    out = []
    for c in yields:
        if c.expr.kind in (E.K_INPUT, E.K_VAR) and c.expr.prop == "*":
            for n in columns:
                out.append(AggCol(c.fun, E.input_prop(n) if c.expr.kind == E.K_INPUT else E.var_prop(c.expr.alias, n)))
        else:
            out.append(c)
    return out


def result_types(cols: List[AggCol]):
    """Collector::getSchema: a root cast's type, else None — the value's own kind (INT for every
    integer payload: a VID or TIMESTAMP column passed through becomes INT)."""
    return [CAST_TYPES[c.expr.op] if c.expr.kind == E.K_CAST else None for c in cols]


def yield_model(inp: Optional[ngql.Interim], st: YieldSentence, types=None):
    """YieldExecutor over an Interim -> (Interim, column types): the input's rows in order, the
    WHERE first, the YIELDs on the rows that pass.  An evaluation error is E_EXECUTION_ERROR."""
    yield_checks(st)
    if st.is_constant():                       # executeConstant: one row, the WHERE is not read
        cols = list(st.yields)
        try:
            row = [evaluate(c.expr) if not (c.fun and c.expr.kind == E.K_PRIMARY and c.expr.value == "*") else "*"
                   for c in cols]
        except EvalError as ex:
            raise GroupError(_lib.E_EXECUTION_ERROR, str(ex))
        row = [groupby.aggregate(c.fun, [v], groupby.type_of_value(v)) if c.fun else v for c, v in zip(cols, row)]
        return ngql.Interim([c.name() for c in cols], [row]), result_types(cols)
    if inp is None:                            # no input at all: an empty result
        return ngql.Interim([c.name() for c in st.yields], []), None
    cols = expand(st.yields, inp.columns)
    names = [c.name() for c in cols]
    if not inp.rows:
        return ngql.Interim(names, []), result_types(cols)
    what = "variable" if st.variables() else "input"
    for n in [n for c in cols for n in c.expr.walk()] + (list(st.where.walk()) if st.where is not None else []):
        if n.kind in (E.K_INPUT, E.K_VAR) and n.prop not in inp.columns:
            raise GroupError(_lib.E_EXECUTION_ERROR, f"column `{n.prop}' not exist in {what}.")
    index = {}
    for i, n in enumerate(inp.columns):
        index.setdefault(n, i)                 # getFieldIndex: the first column of that name
    rows = []
    try:
        for r in inp.rows:
            def get(node, r=r):
                return r[index[node.prop]]
            if st.where is not None and not as_bool_where(evaluate(st.where, get)):
                continue
            rows.append([evaluate(c.expr, get) if not (c.expr.kind == E.K_PRIMARY and c.expr.value == "*" and c.fun)
                         else "*" for c in cols])
    except EvalError as ex:
        raise GroupError(_lib.E_EXECUTION_ERROR, str(ex))
    if not any(c.fun for c in cols):
        return ngql.Interim(names, rows), result_types(cols)
    # whole-input aggregates (the device answers NBG_E_UNSUPPORTED; the fallback runs this loop)
    if not rows:
        raise ModelScope("aggregates over no rows")
    if types is None:
        types = [groupby.type_of_value(v) for v in inp.rows[0]]
    out = []
    for k, c in enumerate(cols):
        vals = [r[k] for r in rows]
        t = types[index[c.expr.prop]] if c.expr.kind in (E.K_INPUT, E.K_VAR) else groupby.type_of_value(vals[0])
        out.append(groupby.aggregate(c.fun, vals, t))
    return ngql.Interim(names, [out]), None


def as_bool_where(v):
    """Expression::asBool of the WHERE value; a string is true when it is empty (Expressions.h:228-241)."""
    return v == "" if isinstance(v, str) else as_bool(v)


# ------------------------------------------------------------------------------------ execution
class Session(setops.Session):
    """setops.Session plus the YIELD sentence, `;`-separated statements and `$var = ...`.  Every
    sentence maps a Value to a Value.  Without `device` everything after the GOs runs in the
    models.  With it, a GO that is followed by a stage (or ends the statement) runs with go_device,
    and every stage whose input is on the device stays there: Engine.group_by, Engine.order_by (an
    adjacent `ORDER BY | LIMIT` is one call), Engine.yield_rows, Engine.set_op; a variable keeps its
    rows on the device too.  The statement fetches once at its end, or where a following
    `| GO FROM $-.x` needs its input on the host.  A YIELD without `$-' / `$var' is the reference's
    executeConstant and runs in the model.  A stage the engine answers with NBG_E_UNSUPPORTED falls
    back to the model over the fetched rows and is recorded in `fallbacks`; `yield_calls` counts the
    YIELDs nbg_yield completed."""

    def __init__(self, backend, device=False):
        super().__init__(backend, device)
        self.values = {}
        self.yield_calls = 0

    def execute(self, text: str) -> ngql.Interim:
        self.set_calls, self.fallbacks, self.yield_calls = [], [], 0
        self.values = {}
        stmts = [(var, parse_statement(s)) for var, s in split_statements(text)]
        last = None
        try:
            for var, tree in stmts:
                self._release(last)
                last = None
                last = self._eval(tree, None)
                if var is not None:
                    old = self.values.pop(var, None)
                    if old is not None:
                        old.free()
                    last.pinned = True
                    self.values[var] = last
            return last.fetch() if last is not None else ngql.Interim([], [])
        finally:
            self._release(last)
            for v in self.values.values():
                v.free()
            self.values = {}

    @staticmethod
    def _release(v):
        if v is not None and not getattr(v, "pinned", False):
            v.free()

    def _source(self, ref, inp):
        if ref[0] == "$-":
            return inp
        if ref[0] not in self.values:
            raise GroupError(_lib.E_EXECUTION_ERROR, f"Variable `{ref[0]}' not defined")
        return self.values[ref[0]].fetch()

    def _pipe(self, parts, inp) -> Value:
        val = Value(inp.columns, interim=inp) if inp is not None else None
        i = 0
        while i < len(parts):
            if not isinstance(parts[i], str):
                nxt = self._eval(parts[i], val.fetch() if val is not None else None)
                self._release(val)
                val = nxt
                i += 1
                continue
            j = i
            while j < len(parts) and isinstance(parts[j], str):
                j += 1
            val = self._sentences([parse_sentence(p) for p in parts[i:j]], val, last=j == len(parts))
            i = j
        return val

    def _sentences(self, sents, val, last) -> Value:
        for st in sents:                  # every executor's prepare() runs before the first execute()
            if isinstance(st, LimitSentence):
                orderby.check_limit(st.offset, st.count)
        i = 0
        while i < len(sents):
            st, step = sents[i], 1
            if isinstance(st, ngql.GoSentence):
                staged = (i + 1 < len(sents) and isinstance(sents[i + 1], STAGES)) or (last and i == len(sents) - 1)
                inp = val.fetch() if val is not None else None
                if self.device and staged and self._device_go(st):
                    new = self._go_stages_rows(st, [], inp)
                else:
                    r = self._go(st, inp)
                    new = Value(r.columns, groupby.go_column_types(st, r.rows), interim=r)
            elif isinstance(st, STAGES):
                src = self._stage_input(st, val)
                on_device = self.device and src is not None and src.rows is not None
                if isinstance(st, YieldSentence) and st.is_constant():
                    on_device = False
                if on_device:
                    new, step = self._stage_device(sents, i, src)
                else:
                    new = self._stage_host(st, src)
            else:
                r = self._find(st, val.fetch() if val is not None else None)
                new = Value(r.columns, None, interim=r)
            self._release(val)
            val = new
            i += step
        return val if val is not None else Value([], interim=ngql.Interim([], []))

    def _stage_input(self, st, val):
        """A YIELD over `$var' reads the variable, whatever is piped in."""
        if not isinstance(st, YieldSentence) or not st.variables():
            return val
        for v in st.variables():
            if v in self.values:
                return self.values[v]
        yield_checks(st)                       # (statuses 3 and 4 come before the variable lookup)
        raise GroupError(_lib.E_EXECUTION_ERROR, f"Variable `{st.variables()[0]}' not defined.")

    def _stage_host(self, st, src) -> Value:
        inp = src.fetch() if src is not None else None
        types = self._types(src, inp) if inp is not None and inp.rows else None
        if isinstance(st, YieldSentence):
            res, rtypes = yield_model(inp, st, types)
            return Value(res.columns, rtypes, interim=res)
        if inp is None:
            names = [y.name() for y in st.yields] if isinstance(st, GroupBySentence) else []
            return Value(names, None, interim=ngql.Interim(names, []))
        if isinstance(st, GroupBySentence):
            res = groupby.group_model(inp, st.groups, st.yields, types)
            return Value(res.columns, None, interim=res)
        if isinstance(st, OrderBySentence):
            return Value(inp.columns, src.types, interim=orderby.order_model(inp, st.factors))
        return Value(inp.columns, src.types, interim=orderby.limit_model(inp, st.offset, st.count))

    def _stage_device(self, sents, i, src):
        """(Value, sentences consumed) of the stage sents[i] over the device rows of `src`."""
        st, names, rows, step = sents[i], src.names, src.rows, 1
        try:
            if isinstance(st, GroupBySentence):
                out = self.b.group_by(rows, names,
                                      [(E.Expr(E.K_FUNC, alias=c.fun, args=[c.expr]) if c.fun else c.expr).encode()
                                       for c in st.groups],
                                      [(c.fun, c.expr.encode(), c.alias) for c in st.yields])
                return Value([c.name() for c in st.yields], None, rows=out), 1
            if isinstance(st, YieldSentence):
                funs = [c.fun for c in st.yields] if any(c.fun for c in st.yields) else None
                out = self.b.yield_rows(rows, names, [c.expr.encode() for c in st.yields],
                                        st.where.encode() if st.where is not None else b"",
                                        [f if f else 0 for f in funs] if funs else None)
                self.yield_calls += 1
                cols = expand(st.yields, names)
                return Value([c.name() for c in cols], result_types(cols), rows=out), 1
            factors, limit = [], None
            if isinstance(st, OrderBySentence):
                factors = st.factors
                if i + 1 < len(sents) and isinstance(sents[i + 1], LimitSentence):
                    step = 2
                    limit = (sents[i + 1].offset, sents[i + 1].count)
            else:
                limit = (st.offset, st.count)
            return Value(names, src.types, rows=self.b.order_by(rows, names, factors, limit)), step
        except NbgError as ex:
            if ex.code != _lib.E_UNSUPPORTED:
                raise
            self.fallbacks.append((type(st).__name__, ex.code))
        new = self._stage_host(st, src)
        if step == 2:
            nxt = self._stage_host(sents[i + 1], new)
            new.free()
            new = nxt
        return new, step


# ------------------------------------------------------------------------------------ comparing
def run_case(session: Session, case):
    """(ok, message) for one yield_golden.json case: the status and the rows as a multiset with
    their kinds (verifyResult sorts both sides)."""
    st, res = session.status(case["query"])
    if st != case["status"]:
        return False, f"status {st} != {case['status']}"
    if st != "SUCCEEDED":
        return True, "failed as expected"
    got, exp = groupby.multiset(res.rows), groupby.multiset(case["expected"])
    return got == exp, "" if got == exp else f"rows {res.rows} != {case['expected']}"

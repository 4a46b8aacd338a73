"""TEST HARNESS: the `FETCH PROP ON <tag>` sentence for the nGQL front end of tests/support
(ngql.py ... yieldpipe.py), a plain-Python model of FetchVerticesExecutor / FetchExecutor
(src/graph/FetchVerticesExecutor.cpp:19-311, src/graph/FetchExecutor.cpp:14-131) as include/nbg.h
restates them for nbg_fetch_vertices, and a session whose device mode keeps the FETCH stage in HBM
beside YIELD, GROUP BY, ORDER BY / LIMIT and the set operators.

The model is the checker of tests/test_gpu_fetch.py; tests/test_fetch_model.py pins it to the
reference's own FetchVerticesTest vectors (tests/golden/fetch_golden.json) first.

Grammar (parser.yy fetch_vertices_sentence):
    FETCH PROP ON label (vid_list | $-.col | $var.col) [YIELD [DISTINCT] yield_columns]
It stands alone, as a pipe stage and after `$var = ...;`.

The model works over TagTables: per tag its id, its latest schema and {vid: row} for the vertices
the storage client finds (a decoded record of the tag, in the part vid % parts + 1).  Expressions are
yieldpipe.evaluate's subset with `tag.prop` reading the found vertex's row.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

from nebula_amd import _lib, expr as E
from nebula_amd.engine import NbgError
from tests.support import groupby, ngql, setops, yieldpipe
from tests.support.groupby import BOOL, DOUBLE, INT, STRING, TIMESTAMP, VID, AggCol, GroupError
from tests.support.setops import PipeNode, SetNode, Value
from tests.support.yieldpipe import CAST_TYPES, EvalError, ModelScope  # noqa: F401  (re-exported)

ALIAS_KINDS = (E.K_ALIAS, E.K_RANK, E.K_DST, E.K_SRCID, E.K_TYPE)
PSEUDO_PROPS = {E.K_RANK: "_rank", E.K_DST: "_dst", E.K_SRCID: "_src", E.K_TYPE: "_type"}


# ------------------------------------------------------------------------------------ parsing
@dataclass
class FetchSentence:
    label: str
    vids: List[int] = field(default_factory=list)
    ref: Optional[tuple] = None               # ("$-", col) or (variable, col)
    yields: Optional[List[AggCol]] = None     # None: no YIELD clause
    distinct: bool = False

    def variables(self):
        return [self.ref[0]] if self.ref is not None and self.ref[0] != "$-" else []


STAGES = yieldpipe.STAGES + (FetchSentence,)


class Parser(yieldpipe.Parser):
    """yieldpipe.Parser plus fetch_vertices_sentence."""

    def primary_sentence(self):
        if self.kw("FETCH"):
            return self.fetch_sentence()
        return super().primary_sentence()

    def fetch_sentence(self):
        self.expect_kw("FETCH")
        self.expect_kw("PROP")
        self.expect_kw("ON")
        kind, label = self.take()
        if kind != "name":
            raise ngql.ParseError(f"expected a tag name, got {label!r}")
        vids, ref = self.vid_list_or_ref()
        s = FetchSentence(label, vids, ref)
        if self.kw("YIELD"):
            self.take()
            if self.kw("DISTINCT"):
                self.take()
                s.distinct = True
            s.yields = self.agg_cols()
            if any(c.fun for c in s.yields):
                raise ngql.ParseError("aggregate functions are not part of a FETCH's YIELD")
        return s


def parse_sentence(text: str):
    p = Parser(text)
    s = p.primary_sentence()
    if p.peek()[0] != "eof":
        raise ngql.ParseError(f"trailing input near {p.peek()[1]!r}")
    return s


def parse_statement(text: str):
    """yieldpipe.parse_statement with the FETCH sentence: the SetNode / PipeNode tree."""
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


# ------------------------------------------------------------------------------------ the model
@dataclass
class TagTable:
    """One tag as the storage client sees it: `rows` holds the vertices it finds."""
    tag_id: int
    schema: List[tuple]                        # [(prop name, groupby type name)], latest version
    rows: Dict[int, list]

    def index(self, prop):
        for i, (n, _) in enumerate(self.schema):
            if n == prop:
                return i
        return -1


def columns_of(st: FetchSentence, table: TagTable) -> List[AggCol]:
    """FetchExecutor::setupColumns: without a YIELD clause, every column of the latest schema."""
    if st.yields is not None:
        return list(st.yields)
    return [AggCol("", E.edge_prop(st.label, n)) for n, _ in table.schema]


def result_types(cols: List[AggCol], table: TagTable):
    """FetchExecutor::prepareYield: a bare `tag.prop' takes the schema's field type, a root cast
    the cast's type, anything else None — the value's own kind."""
    out = []
    for c in cols:
        if c.expr.kind == E.K_ALIAS and table.index(c.expr.prop) >= 0:
            out.append(table.schema[table.index(c.expr.prop)][1])
        elif c.expr.kind == E.K_CAST:
            out.append(CAST_TYPES[c.expr.op])
        else:
            out.append(None)
    return out


def _as_input(e: E.Expr) -> E.Expr:
    """The tree with every `tag.prop' as `$-.prop', so yieldpipe.evaluate's getter reads it."""
    if e.kind == E.K_ALIAS:
        return E.input_prop(e.prop)
    if not e.args:
        return e
    return E.Expr(e.kind, op=e.op, value=e.value, alias=e.alias, prop=e.prop, ref=e.ref, args=[_as_input(a) for a in e.args])


def input_vids(st: FetchSentence, inp: ngql.Interim, types=None):
    """Status 6's first part, getVIDs -> RowReader::getVid: the vid column of a non-empty input;
    INT and VID columns only."""
    col = st.ref[1]
    ok = col in inp.columns
    if ok:
        k = inp.columns.index(col)
        t = types[k] if types is not None and types[k] is not None else groupby.type_of_value(inp.rows[0][k])
        ok = t in (INT, VID)
    if not ok:
        raise GroupError(_lib.E_EXECUTION_ERROR, f"Column `{col}' not found")
    return [r[k] for r in inp.rows]


def fetch_model(st: FetchSentence, tables: Dict[str, TagTable], inp: Optional[ngql.Interim], types=None):
    """FetchVerticesExecutor over a vid list (inp None) or an Interim -> (Interim, column types),
    in include/nbg.h's status order.  One row per input row whose vid the table holds, in the
    input's order; under DISTINCT the first of each distinct row."""
    # 3. prepareClauses / prepareVids
    table = tables.get(st.label)
    if table is None:
        raise GroupError(_lib.E_EXECUTION_ERROR, f"{st.label} tag schema not exist.")
    if st.ref is not None and st.ref[1] == "*":
        raise GroupError(_lib.E_EXECUTION_ERROR, "Cant not use `*' to reference a vertex id column.")
    cols = columns_of(st, table)
    names = [c.name() for c in cols]
    # 4. prepareYield
    nodes = [n for c in cols for n in c.expr.walk()]
    if any(n.kind in (E.K_SRC, E.K_DESTP) for n in nodes):
        raise GroupError(_lib.E_SYNTAX_ERROR, "tag.prop and edgetype.prop are supported in fetch sentence.")
    if any(n.kind in (E.K_INPUT, E.K_VAR) for n in nodes):
        raise GroupError(_lib.E_SYNTAX_ERROR, "`$-' and `$variable' not supported in fetch yet.")
    props = [(n.alias, PSEUDO_PROPS.get(n.kind, n.prop)) for n in nodes if n.kind in ALIAS_KINDS]
    for alias, prop in props:
        if alias != st.label:
            raise GroupError(_lib.E_SYNTAX_ERROR, f"Near [{alias}.{prop}], tag or edge should be declared in statement first.")
    # 5. setupVids, onEmptyInputs
    if st.ref is None:
        vids = list(st.vids)
    else:
        if inp is None or not inp.rows:
            return ngql.Interim(names, []), result_types(cols, table)
        vids = input_vids(st, inp, types)
    if not vids:
        return ngql.Interim(names, []), result_types(cols, table)
    if not props:
        raise GroupError(_lib.E_EXECUTION_ERROR, "No props declared.")
    if any(table.index(p) < 0 for _, p in props):
        raise GroupError(_lib.E_EXECUTION_ERROR, "Get props failed")
    # 8. processResult
    exprs = [_as_input(c.expr) for c in cols]
    rows = []
    try:
        for v in vids:
            rec = table.rows.get(v)
            if rec is None:
                continue

            def get(node, rec=rec):
                return rec[table.index(node.prop)]
            rows.append([yieldpipe.evaluate(e, get) for e in exprs])
    except EvalError as ex:
        raise GroupError(_lib.E_EXECUTION_ERROR, str(ex))
    if st.distinct:
        seen = {}
        for r in rows:
            seen.setdefault(setops.row_key(r, by_bits=True), r)
        rows = list(seen.values())
    return ngql.Interim(names, rows), result_types(cols, table)


# ------------------------------------------------------------------------------------ execution
class Session(yieldpipe.Session):
    """yieldpipe.Session plus the FETCH sentence.  `tables` maps a tag name to its TagTable (the
    model's data and, through tag_id, the binding's name resolution).  With `device`, a FETCH whose
    input is on the device stays there (Engine.fetch_vertices over the rows); a FETCH over a
    literal vid list, or over rows the host holds, runs on the device through the in == NULL path;
    the statement still fetches once at its end.  A FETCH the engine answers with NBG_E_UNSUPPORTED falls back to the model over
    the fetched rows and is recorded in `fallbacks`; `fetch_calls` counts the FETCHes
    nbg_fetch_vertices completed and `fetch_paths` says how each got its vids: "rows" (a device
    handle as `in`), "list" (the sentence's own vid list) or "host rows" (a piped input the host
    held, sent as a list)."""

    def __init__(self, backend, tables: Dict[str, TagTable], device=False):
        super().__init__(backend, device)
        self.tables = tables
        self.fetch_calls = 0
        self.fetch_paths = []

    def execute(self, text: str) -> ngql.Interim:
        self.set_calls, self.fallbacks, self.yield_calls, self.fetch_calls = [], [], 0, 0
        self.fetch_paths = []
        self.values = {}
        stmts = [(var, parse_statement(s)) for var, s in yieldpipe.split_statements(text)]
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
            val = self._fetch_sentences([parse_sentence(p) for p in parts[i:j]], val, last=j == len(parts))
            i = j
        return val

    def _fetch_sentences(self, sents, val, last) -> Value:
        """Runs of sentences between FETCHes go through yieldpipe.Session._sentences; a GO right
        in front of a FETCH counts as staged, so it stays on the device."""
        i = 0
        while i < len(sents):
            if isinstance(sents[i], FetchSentence):
                new = self._fetch(sents[i], val)
                self._release(val)
                val = new
                i += 1
                continue
            j = i
            while j < len(sents) and not isinstance(sents[j], FetchSentence):
                j += 1
            val = self._sentences(sents[i:j], val, last=(last and j == len(sents)) or j < len(sents))
            i = j
        return val if val is not None else Value([], interim=ngql.Interim([], []))

    def _fetch(self, st: FetchSentence, val) -> Value:
        src = val
        if st.variables():
            if st.variables()[0] not in self.values:
                fetch_model(st, self.tables, ngql.Interim([], []))      # (statuses 3 and 4 come first)
                raise GroupError(_lib.E_EXECUTION_ERROR, f"Variable `{st.variables()[0]}' not defined")
            src = self.values[st.variables()[0]]
        table = self.tables.get(st.label)
        if self.device:
            tag_id = table.tag_id if table is not None else -1
            ys = [c.expr.encode() for c in st.yields] if st.yields is not None else []
            try:
                if st.ref is not None and src is not None and src.rows is not None:
                    path = "rows"
                    out = self.b.fetch_vertices(src.rows, src.names, st.ref[1], tag_id, ys, st.distinct)
                else:
                    path = "list" if st.ref is None else "host rows"
                    # a vid list, or a piped input the host holds (a GO the device path does not
                    # take): its vid column goes through the in == NULL path, after the checks
                    # that come before it
                    vids = st.vids
                    if st.ref is not None:
                        inp = src.fetch() if src is not None else None
                        vids = []
                        if inp is not None and inp.rows:
                            fetch_model(st, self.tables, ngql.Interim(inp.columns, []))     # statuses 3 and 4
                            vids = input_vids(st, inp, self._types(src, inp))
                    out = self.b.fetch_vertices(vids, [], "", tag_id, ys, st.distinct)
            except NbgError as ex:
                if ex.code != _lib.E_UNSUPPORTED:
                    raise
                self.fallbacks.append(("FetchSentence", ex.code))
            else:
                self.fetch_calls += 1
                self.fetch_paths.append(path)
                cols = columns_of(st, table)
                return Value([c.name() for c in cols], result_types(cols, table), rows=out)
        inp = src.fetch() if src is not None else None
        types = self._types(src, inp) if inp is not None and inp.rows else None
        res, rtypes = fetch_model(st, self.tables, inp, types)
        return Value(res.columns, rtypes, interim=res)


# ------------------------------------------------------------------------------------ comparing
def nba_tables(data, tag_ids) -> Dict[str, TagTable]:
    """The TraverseTestBase data set's tags (tests/golden/nba.json): player(name, age), team(name)."""
    return {
        "player": TagTable(tag_ids["player"], [("name", STRING), ("age", INT)],
                           {p["vid"]: [p["name"], p["age"]] for p in data["players"]}),
        "team": TagTable(tag_ids["team"], [("name", STRING)], {t["vid"]: [t["name"]] for t in data["teams"]}),
    }


def run_case(session: Session, case):
    """(ok, message) for one fetch_golden.json case: status, column names where the reference's
    test asserts them, and the rows — in order where the reference compares them so (verifyResult
    without sorting), else as a multiset with their kinds."""
    st, res = session.status(case["query"])
    if st != case["status"]:
        return False, f"status {st} != {case['status']}"
    if st != "SUCCEEDED":
        return True, "failed as expected"
    if "col_names" in case and res.columns != case["col_names"]:
        return False, f"columns {res.columns} != {case['col_names']}"
    if case.get("ordered"):
        got, exp = [list(r) for r in res.rows], [list(r) for r in case["expected"]]
    else:
        got, exp = groupby.multiset(res.rows), groupby.multiset(case["expected"])
    return got == exp, "" if got == exp else f"rows {res.rows} != {case['expected']}"

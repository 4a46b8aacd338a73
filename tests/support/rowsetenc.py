"""RowSetWriter restated for test assertions (src/dataman/RowSetWriter.cpp:21-33): the bytes of an
InterimResult's rows, every row a RowWriter row (kvgen.encode_row, pinned to the reference's own
vectors by tests/test_oracle_storage.py) behind the varint of its length.  The yardstick of
nbg_rows_encode; it shares no code with it."""
from nebula_amd import kvgen
from nebula_amd.kvgen import _varint


def encode_rowset(types, rows) -> bytes:
    schema = [("", t) for t in types]
    out = []
    for row in rows:
        r = kvgen.encode_row(schema, row, 0)
        out.append(_varint(len(r)) + r)
    return b"".join(out)

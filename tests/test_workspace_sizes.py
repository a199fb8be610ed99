"""Workspace queries against the values recorded from the library before the
layouts became the queries' only definition (tests/golden/workspace_sizes.json,
tests/golden/make_golden_workspace.py).  Pure host: runs without a GPU."""
import json
import os

import pytest

from conftest import GOLDEN

ROWS = json.load(open(os.path.join(GOLDEN, "workspace_sizes.json")))
# Growth can only be alignment padding: under 256 bytes per region where the
# order of the regions changed or a region is now always taken, and no layout
# has 32 regions.
SLACK = 8192


def test_table_covers_every_query():
    from pyabc_amd import _native as nat
    queries = {n for n in nat.SIGNATURES if n.endswith("_workspace")}
    assert {q for q, _, _ in ROWS} == queries


@pytest.mark.parametrize("query", sorted({q for q, _, _ in ROWS}))
def test_no_query_grows(query):
    from pyabc_amd import _native as nat
    for q, args, parent in ROWS:
        if q != query:
            continue
        new = nat.query(q, *args)
        assert new <= parent + SLACK, (q, args, new, parent)
        # a query never returns less than its layout's trailing 256 bytes,
        # except where the parent answered 0 for arguments it rejects
        assert new >= 256 or parent == 0, (q, args, new)
        assert (new == 0) == (parent == 0), (q, args, new, parent)

"""The clock logic of tests/stream_audit.py on fake streams (no GPU), and the documentation test of the switch table: every
`MINDPOSE_*` / `MP_*` name the package or bench.py reads has a row in INTEGRATION.md "Switches (environment)" - an undocumented
switch (`MINDPOSE_TRAIN_CHAIN_MODULES`) is how a broken combination of two of them went unnoticed."""
import glob
import os
import re

from tests.stream_audit import OrderAudit, StreamClocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_consume_on_another_stream_without_a_wait_is_flagged():
    a = OrderAudit()
    a.produce("buf", "A", "stage3.0.fuse_layers.1")
    assert not a.consume("buf", "B", "stage3.1.branches.1.0")
    assert len(a.violations) == 1
    v = a.violations[0]
    assert (v.where, v.producer, v.consumer, v.produced_at) == ("stage3.1.branches.1.0", "A", "B", "stage3.0.fuse_layers.1")
    assert "stage3.1.branches.1.0" in a.report() and "producer stream A" in a.report() and "consumer stream B" in a.report()


def test_same_stream_and_wait_first_pass():
    a = OrderAudit()
    a.produce("buf", "A", "p")
    assert a.consume("buf", "A", "c")  # stream order
    a.wait("B", "A")
    assert a.consume("buf", "B", "c")
    assert not a.violations and a.checked == 2 and a.edges == [("B", "A")]


def test_order_is_transitive_through_a_third_stream():
    a = OrderAudit()
    a.produce("buf", "A", "p")
    a.wait("C", "A")
    a.produce("other", "C", "q")
    a.wait("B", "C")
    assert a.consume("buf", "B", "c") and a.consume("other", "B", "c")
    assert not a.violations
    # ... but not against the direction of the edges
    a.produce("late", "B", "r")
    assert not a.consume("late", "A", "c")


def test_a_wait_issued_before_the_producer_ran_does_not_count():
    a = OrderAudit()
    a.wait("B", "A")             # B is ordered behind what A had launched THEN: nothing
    a.produce("buf", "A", "p")
    assert not a.consume("buf", "B", "c")
    # a chain whose first edge is too early does not count either
    b = OrderAudit()
    b.wait("C", "A")
    b.produce("buf", "A", "p")
    b.wait("B", "C")
    assert not b.consume("buf", "B", "c")
    # the second of two launches is not covered by a wait between them
    c = OrderAudit()
    c.produce("one", "A", "p")
    c.wait("B", "A")
    c.produce("two", "A", "p")
    assert c.consume("one", "B", "c") and not c.consume("two", "B", "c")


def test_unknown_buffers_pass_and_a_later_producer_replaces_the_earlier():
    a = OrderAudit()
    assert a.consume("input image", "B", "c") and a.checked == 0
    a.produce("buf", "A", "p")
    a.produce("buf", "B", "q")   # written again on B: B's launch is the one a reader must follow
    assert a.consume("buf", "B", "c") and not a.consume("buf", "A", "c")


def test_finish_wants_an_edge_from_every_stream_that_produced_something():
    a = OrderAudit()
    a.produce("x", "main", "p")
    a.produce("y", "side0", "stage4.2.branches.1.3")
    a.produce("z", "side1", "stage4.2.branches.2.3")
    a.wait("main", "side0")
    a.finish("main")
    assert [(v.producer, v.consumer, v.what) for v in a.violations] == [("side1", "main", "stream left unjoined")]
    assert a.violations[0].produced_at == "stage4.2.branches.2.3"
    a.violations.clear()
    a.wait("main", "side1")
    a.finish("main")
    assert not a.violations
    # a launch on a side stream after its join leaves it unjoined again
    a.produce("w", "side0", "late")
    a.finish("main")
    assert len(a.violations) == 1 and a.violations[0].producer == "side0"


def test_clocks_merge_component_wise():
    c = StreamClocks()
    c.tick("A"), c.tick("A"), c.tick("B")
    c.wait("C", "A")
    c.wait("C", "B")
    assert c.sees("C", ("A", 2)) and c.sees("C", ("B", 1)) and not c.sees("C", ("A", 3)) and not c.sees("B", ("A", 1))
    c.wait("A", "A")  # a stream waiting for itself is a no-op
    assert c.now("A") == 2


# ---- the switch table ----------------------------------------------------------------------------------------------------------------

_PY_READ = re.compile(r"""(?:os\.environ\.get|os\.environ\.setdefault|os\.getenv|env_on)\(\s*['"]((?:MINDPOSE|MP)_[A-Z0-9_]+)['"]""")
_C_READ = re.compile(r'''(?:getenv|knob)\(\s*"((?:MINDPOSE|MP)_[A-Z0-9_]+)"''')  # knob() is csrc/common.h's guarded getenv


def _names_read():
    found = {}
    py = glob.glob(os.path.join(ROOT, "mindpose_amd", "**", "*.py"), recursive=True) + [os.path.join(ROOT, "bench.py")]
    for path in sorted(py):
        with open(path) as fh:
            for m in _PY_READ.finditer(fh.read()):
                found.setdefault(m.group(1), os.path.relpath(path, ROOT))
    for path in sorted(glob.glob(os.path.join(ROOT, "mindpose_amd", "csrc", "*"))):
        if path.endswith((".hip", ".h")):
            with open(path) as fh:
                for m in _C_READ.finditer(fh.read()):
                    found.setdefault(m.group(1), os.path.relpath(path, ROOT))
    return {n: p for n, p in found.items() if not n.startswith("MINDPOSE_TEST_")}


def _switch_table():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        text = fh.read()
    start = text.index("## Switches (environment)")
    nxt = text.find("\n## ", start + 1)
    section = text[start:nxt if nxt > 0 else len(text)]
    return [ln for ln in section.splitlines() if ln.startswith("|")]


def test_every_environment_name_the_code_reads_has_a_row_in_the_switch_table():
    names = _names_read()
    assert len(names) >= 60 and "MINDPOSE_TRAIN_CHAIN_MODULES" in names and "MP_BN16_COOP_MAX" in names, sorted(names)  # the scan works
    rows = _switch_table()
    assert len(rows) >= 40
    documented = set()
    for row in rows:  # (a sub-switch may sit in the effect cell of the row of the switch it refines: MINDPOSE_BN_PRE_CH)
        documented |= set(re.findall(r"(?:MINDPOSE|MP)_[A-Z0-9_]+", row))
    missing = {n: p for n, p in names.items() if n not in documented}
    assert not missing, f"read by the code, no row in INTEGRATION.md 'Switches (environment)': {missing}"

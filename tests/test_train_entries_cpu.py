"""The four trainers' entry points before their first HIP call: work-space sizes and refusals against the integers of
tests/golden/train_entries.json (written by tests/golden/make_golden_train_entries.py, whose tables and row runner are
used here).  No row reaches a HIP call, so the module needs no GPU: every refusal row passes a work space of 0 bytes, and
the work-space check is the last one an entry makes."""
import importlib.util
import json
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
_spec = importlib.util.spec_from_file_location("make_golden_train_entries", GOLDEN / "make_golden_train_entries.py")
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

TRAINERS = list(gen.TRAINERS)


@pytest.fixture(scope="module")
def L():
    return gen.load_lib(GOLDEN.parents[1])


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "train_entries.json").read_text())


def _valid_size(L, trainer):
    t = gen.TRAINERS[trainer]
    return gen.sizes_call(L, t["stretch"], gen.make_config(L, trainer, {}), gen.N, gen.N_VAL, None, 0)


@pytest.mark.parametrize("trainer", TRAINERS)
def test_workspace_bytes(L, golden, trainer):
    rows = golden["workspace"][trainer]
    assert [r[:6] for r in rows] == [list(c) for c in gen.workspace_cells(trainer)], "the fixture's table has gaps"
    for want in rows:
        assert want[6] > 0, want
        assert gen.workspace_row(L, trainer, tuple(want[:6])) == want


@pytest.mark.parametrize("trainer", TRAINERS)
def test_fixture_is_complete(L, golden, trainer):
    rows = [r for r in golden["refusals"] if r["trainer"] == trainer]
    keys = ("trainer", "entry", "case", "fields", "cfg", "n", "n_val", "options", "patience", "null", "ws")
    assert [{k: r[k] for k in keys} for r in rows] == list(gen.refusal_cases(L, trainer))
    t = gen.TRAINERS[trainer]
    for entry in t["train"] + t["grads"] + [t["stretch"]]:
        covered = {f for r in rows if r["entry"] == entry and r["case"] == "limit" for f in r["fields"]}
        assert covered == set(gen.config_fields(L, trainer)), entry
    for r in rows:
        assert r["rc"] == -1 if r["entry"].endswith("_workspace_bytes") else r["rc"] > 0, r


@pytest.mark.parametrize("trainer", TRAINERS)
def test_refusals(L, golden, trainer):
    t = gen.TRAINERS[trainer]
    valid = _valid_size(L, trainer)
    assert valid > 0
    for row in (r for r in golden["refusals"] if r["trainer"] == trainer):
        assert gen.run_refusal(L, row) == row["rc"], row
        said = L.last_error()
        name = t["says"] + ("_loss_grads" if row["entry"] in t["grads"] else "_train")
        assert said and name in said, (row, said)
        assert _valid_size(L, trainer) == valid, row  # the next valid call still answers

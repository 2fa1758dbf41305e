"""Every host dataset class of pssr2_amd/data.py against the records in tests/golden/data_protocol.json, which
tools/gen_golden_data_protocol.py wrote from the commit before the classes were put on one shared base: ``len``, ``val_idx``, ``repr``,
names, a digest of every item (``compact`` off and on; index order, one permutation, ``pp=True``), the ``random`` state the passes
leave, every constructor / index error and warning.  The tool's ``records()`` is run again here and compared for equality."""
import importlib.util
import json
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("gen_golden_data_protocol", ROOT / "tools" / "gen_golden_data_protocol.py")
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def recorded():
    return json.loads((ROOT / "tests" / "golden" / "data_protocol.json").read_text())


@pytest.fixture(scope="module")
def recomputed(tool, tmp_path_factory):
    return json.loads(json.dumps(tool.records(tmp_path_factory.mktemp("data_protocol"))))          # through json: tuples become lists


def test_the_same_cases_are_recorded(recorded, recomputed):
    for section in ("cases", "errors", "warnings"):
        assert sorted(recomputed[section]) == sorted(recorded[section]), section
    assert all(message is not None for message in recorded["errors"].values())


@pytest.mark.parametrize("key", ["len", "val_idx", "repr", "names", "printed", "warnings", "items_compact_False", "items_compact_True",
                                 "random_state_compact_False", "random_state_compact_True"])
def test_cases_equal_the_records(recorded, recomputed, key):
    for name, want in recorded["cases"].items():
        assert recomputed["cases"][name].get(key) == want.get(key), (name, key)
        assert (key in want) or name == "SlidingArrayDataset", (name, key)


def test_errors_and_warnings_equal_the_records(recorded, recomputed):
    for name, want in recorded["errors"].items():
        assert recomputed["errors"][name] == want, name
    assert recomputed["warnings"] == recorded["warnings"]


def test_both_kinds_of_item_occur(recorded):
    """The records are worth comparing: training and validation items, several orientations, uint8 items in compact mode."""
    for name, rec in recorded["cases"].items():
        n = rec["len"]
        assert len(rec["items_compact_False"]) == 3 * n and rec["items_compact_False"] != rec["items_compact_True"], name
        if 0 < len(rec["val_idx"]) < n:
            first, pp = rec["items_compact_False"][:n], rec["items_compact_False"][2 * n:]
            assert any(a != b for a, b in zip(first, pp)), name          # a training item was rotated
            assert all(first[i] == pp[i] for i in rec["val_idx"]) or "gaussian" in name, name
            assert rec["random_state_compact_False"] == rec["random_state_compact_True"]

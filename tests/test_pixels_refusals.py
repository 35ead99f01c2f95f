"""What libmodle_pixels.so refuses on the host -- before its first HIP call, so without a device -- is what it
refused before its one-call forms were given one body each: per case of tools/pixels_refusals.py (the sixteen
modle_pixels_*_to_host / _coarse_*_to_host, the two that compare bands, and the forms that enqueue and refuse
overlapping arrays) the return code, the message byte for byte, and which output pointers were nulled.
tests/golden/pixels_refusals.json was written by that tool from the library built from the commit BEFORE the
consolidation, never from the code under test; a change of a contract of include/modle_pixels.h regenerates it from
the library before that change and edits the cases it means to change."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pixels_refusals.json")


def _tool():
    spec = importlib.util.spec_from_file_location("pixels_refusals", os.path.join(ROOT, "tools", "pixels_refusals.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def tables():
    from modle_amd import pixels

    # the package loads the library first: one HIP runtime per process, torch's where there is one (_lib.py);
    # the tool then opens the same loaded library again, with function objects of its own
    pixels.lib()
    with open(GOLDEN) as f:
        want = json.load(f)
    return _tool().run(pixels.SO_PATH), want


def test_the_table_covers_every_one_call_form_and_the_overlap_rules(tables):
    _, want = tables
    names = {case.split(":")[0] for case in want}
    stems = ("to_host", "marginals_to_host", "insulation_to_host", "dots_to_host", "dot_hist_to_host",
             "dots_fdr_to_host", "pileup_to_host", "rescale_to_host")
    assert {"modle_pixels_" + s for s in stems} | {"modle_pixels_coarse_" + s for s in stems} <= names
    assert {"modle_pixels_" + s for s in ("pileup", "rescale", "dots", "dot_hist", "dots_fdr", "marginals", "sample",
                                          "stripes", "scc", "band_check", "band_fill")} <= names
    assert all(v["rc"] in (-1, -3) for v in want.values())  # refusals only: ARG, and RANGE of the bin ids
    coarse = [c for c in want if c.startswith("modle_pixels_coarse_")]
    assert sum(c.endswith(": factor == 1") for c in coarse) == 8
    # the irregularities of the parent are part of the record: the forms that return pixels leave their outputs
    # alone on a refusal, the others null them before they look at anything
    assert set(want["modle_pixels_coarse_to_host: factor == 1"]["outputs"].values()) == {"kept"}
    assert set(want["modle_pixels_coarse_dots_to_host: factor == 1"]["outputs"].values()) == {"kept"}
    assert set(want["modle_pixels_coarse_rescale_to_host: null handle"]["outputs"].values()) == {"null"}


def test_every_refusal_is_what_it_was(tables):
    got, want = tables
    assert sorted(got) == sorted(want)
    different = {case: (got[case], want[case]) for case in want if got[case] != want[case]}
    assert not different, different

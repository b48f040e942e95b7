"""The R-CNN and RetinaNet graphs against the manifest recorded before their code was split into stages (tests/golden/graph_manifest.json, written by
tools/graph_manifest.py at the commit the file names): per form of tests/graph_forms.py the stage marks, the op and conv statistics, the conv launches in
order, the engine's memory, the named buffers and the hash of the detections, each with exact equality."""
import json
import os

import pytest

import graph_forms as gf

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_manifest.json")) as _f:
    MANIFEST = json.load(_f)


def test_manifest_covers_every_form_and_keeps_every_hash():
    assert sorted(MANIFEST["forms"]) == sorted(f["name"] for f in gf.FORMS)
    assert len(MANIFEST["recorded_at"]) == 40
    assert MANIFEST["hash_dropped"] == []
    for name, rec in MANIFEST["forms"].items():
        assert all(c >= 1 for step in rec["counts"] for c in step), name   # a hash over no detections pins nothing


@pytest.mark.parametrize("form", gf.FORMS, ids=lambda f: f["name"])
def test_form_equals_the_manifest(ffi, capfd, form):
    want = gf.unpack(MANIFEST, form["name"])
    got = gf.run_form(form, capfd.readouterr, lambda: capfd.readouterr().err)
    assert got.pop("hash_repeat") == got["hash"], "two runs of one engine disagree"
    if form["name"] in MANIFEST["hash_dropped"]:
        del got["hash"]
    got = json.loads(json.dumps(got))
    assert sorted(got) == sorted(want)
    for field in sorted(want):
        assert got[field] == want[field], field

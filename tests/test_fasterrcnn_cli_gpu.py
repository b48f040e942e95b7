"""`python -m isegmi.cli test_net` with the faster_rcnn yamls and `MODEL.WEIGHT random`, end to end at a small test size: bbox-only COCO json, and with
`--gt` the `bbox` summary alone."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _images(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    src = tmp_path / "in"
    src.mkdir()
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (90 + 10 * i, 120, 3)).astype(np.uint8)).save(src / ("im%d.png" % i))
    return src


def test_cli_test_net_writes_bbox_json_and_prints_only_the_bbox_summary(ffi, tmp_path, capsys):
    from isegmi import cli
    src = _images(tmp_path)
    yaml = os.path.join(ROOT, "configs", "e2e_faster_rcnn_R_50_FPN_1x.yaml")
    args = ["test_net", "--config-file", yaml, "--images", str(src), "--output", str(tmp_path / "b.json")]
    opts = ["MODEL.WEIGHT", "random", "INPUT.MIN_SIZE_TEST", "160", "INPUT.MAX_SIZE_TEST", "256"]
    out = cli.main(args + opts)
    back = json.load(open(tmp_path / "b.json"))
    assert len(back) == len(out) > 0 and {r["image_id"] for r in back} <= {0, 1}
    assert all(set(r) == {"image_id", "category_id", "bbox", "score"} for r in back)
    # the annotation file is the result list itself: every detection finds its box
    gt = {"images": [{"id": i, "height": 90 + 10 * i, "width": 120} for i in range(2)],
          "categories": [{"id": c, "name": str(c)} for c in sorted({r["category_id"] for r in back})],
          "annotations": [{"id": k + 1, "image_id": r["image_id"], "category_id": r["category_id"], "iscrowd": 0, "bbox": r["bbox"],
                           "area": r["bbox"][2] * r["bbox"][3]} for k, r in enumerate(back)]}
    (tmp_path / "gt.json").write_text(json.dumps(gt))
    capsys.readouterr()
    again = cli.main(args + ["--gt", str(tmp_path / "gt.json")] + opts)
    printed = capsys.readouterr().out
    assert again == out
    assert "COCO bbox evaluation:" in printed and "COCO segm evaluation:" not in printed


def test_cli_test_net_runs_the_gn_faster_yaml(ffi, tmp_path):
    from isegmi import cli
    src = _images(tmp_path)
    yaml = os.path.join(ROOT, "configs", "e2e_faster_rcnn_R_50_FPN_Xconv1fc_1x_gn.yaml")
    out = cli.main(["test_net", "--config-file", yaml, "--images", str(src), "--output", str(tmp_path / "g.json"),
                    "MODEL.WEIGHT", "random", "INPUT.MIN_SIZE_TEST", "160", "INPUT.MAX_SIZE_TEST", "256"])
    back = json.load(open(tmp_path / "g.json"))
    assert len(back) == len(out) > 0 and all("segmentation" not in r and len(r["bbox"]) == 4 for r in back)

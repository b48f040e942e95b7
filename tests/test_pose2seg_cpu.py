"""Pose2Seg without a GPU: the CPU restatement (tests/pose2seg_ref.py) against upstream's torch ops and known answers, the letterbox
matrices, the keypoint-json reader and the CLI's argument parsing."""
import json

import numpy as np
import pytest

import pose2seg_ref as ref
from isegmi.weights import pose_templates


@pytest.mark.parametrize("align_corners", [0, 1])
def test_affine_align_is_upstreams_affine_grid_plus_grid_sample(align_corners):
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F
    rng = np.random.default_rng(align_corners)
    feat = rng.standard_normal((128, 128, 8)).astype(np.float32)
    H = [0.9, 0.15, -20.0, -0.1, 1.1, -15.0, 0.0, 0.0, 1.0]
    G = np.array(ref.align_matrix(H, align_corners)[:6]).astype(np.float32)
    got = ref.affine_align(feat, G)
    A = np.array([[2 / 128, 0, -1], [0, 2 / 128, -1], [0, 0, 1]], np.float64)
    theta = np.linalg.inv(A @ np.array(H).reshape(3, 3) @ np.linalg.inv(A))[:2]
    grid = F.affine_grid(torch.tensor(theta[None]), (1, 8, 128, 128), align_corners=bool(align_corners))
    want = F.grid_sample(torch.tensor(feat.transpose(2, 0, 1)[None].astype(np.float64)), grid, mode="bilinear", padding_mode="zeros",
                         align_corners=bool(align_corners))[0].numpy().transpose(1, 2, 0)[:64, :64]
    assert np.abs(want).max() > 0.1
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())


def _exact_image_of(template, A, m1):
    """keypoints (fp64) whose feature-space image under A is exactly `template`'s points"""
    M = np.vstack([np.array(A).reshape(2, 3), [0, 0, 1]])
    kf = np.linalg.solve(M, np.vstack([template[:, 0], template[:, 1], np.ones(17)]))
    m21 = np.diag([0.25, 0.25, 1.0]) @ np.vstack([np.array(m1).reshape(2, 3), [0, 0, 1]])
    ki = np.linalg.solve(m21, kf)
    return np.stack([ki[0], ki[1], np.full(17, 2.0)], 1)


def test_fit_recovers_an_exact_affine_of_template_1():
    tp = pose_templates()
    A = [0.8, 0.12, -30.0, -0.07, 0.95, -12.5]
    m1 = ref.m1_of(480, 640)
    k = _exact_image_of(tp[1].astype(np.float64), A, m1)
    f = ref.fit(k, m1, tp)
    assert f["t"] == 1
    np.testing.assert_allclose(f["m3"], A, rtol=0, atol=1e-9)
    assert f["err"] < 1e-18


def test_fit_ties_go_to_the_lowest_template():
    tp = pose_templates()
    tp2 = np.stack([tp[2], tp[0], tp[0]])
    k = _exact_image_of(tp[0].astype(np.float64), [1.0, 0.0, 3.0, 0.0, 1.0, 4.0], ref.m1_of(512, 512))
    assert ref.fit(k, ref.m1_of(512, 512), tp2)["t"] == 1


def test_fit_fallbacks():
    tp = pose_templates()
    m1 = ref.m1_of(512, 512)      # identity letterbox: feature = image / 4
    k = np.zeros((17, 3), np.float32)
    k[3] = (40, 80, 2); k[9] = (100, 200, 1)    # two visible: fewer than 3 usable points
    f = ref.fit(k, m1, tp)
    assert f["t"] == -1
    side = max(60 / 4, 120 / 4) * 1.2
    s = 64.0 / side
    np.testing.assert_allclose(f["m3"], [s, 0, 32 - s * 17.5, 0, s, 32 - s * 35.0], atol=1e-12)
    k = np.zeros((17, 3), np.float32)
    for j in range(17):
        k[j] = (8 * j + 4, 8 * j + 4, 2)        # collinear: the normal equations are singular
    f = ref.fit(k, m1, tp)
    assert f["t"] == -1 and f["m3"][0] == f["m3"][4]
    k = np.zeros((17, 3), np.float32)
    k[5] = (100, 100, 2)                         # one point: the box is squared to the 8 px minimum
    assert ref.fit(k, m1, tp)["m3"][0] == 8.0
    f = ref.fit(np.zeros((17, 3), np.float32), m1, tp)   # nothing visible: the whole 128 x 128 map at scale 1/2
    assert f["t"] == -1 and list(f["m3"]) == [0.5, 0, 0, 0, 0.5, 0]
    assert np.all(f["mmask"] == np.float32([0.125, 0, 0, 0, 0.125, 0]))


def test_skeleton_heatmap_peak_and_radius():
    k = np.zeros((17, 3), np.float32)
    k[0] = (32, 32, 2)
    s = ref.skeleton(k)
    assert s[32, 32, 0] == 1.0
    y, x = np.mgrid[0:64, 0:64]
    d = np.sqrt((x - 32.0) ** 2 + (y - 32.0) ** 2)
    r = np.sqrt(2 * 9 * 4.6052)
    assert np.all(s[..., 0][d > r + 1e-3] == 0) and np.all(s[..., 0][d < r - 1e-3] > 0)
    assert not s[..., 1:].any()


def test_skeleton_limb_band():
    k = np.zeros((17, 3), np.float32)
    k[5] = (10, 20, 2); k[6] = (40, 20, 2)       # limb [6, 7] (1-based) = index 7: left -> right shoulder, horizontal
    s = ref.skeleton(k)
    l = ref.LIMBS.index([6, 7])
    vx, vy = s[..., 17 + 2 * l], s[..., 18 + 2 * l]
    assert np.all(vy == 0)
    on = vx == 1
    assert on[20, 9:41].all() and on.sum() == 32         # row 20 only (|perp| < 1), x in [rint(9), rint(41))
    others = np.delete(s[..., 17:], [2 * l, 2 * l + 1], axis=2)
    assert not others.any()
    k[6, 2] = 0                                   # an invisible end: no limb
    assert not ref.skeleton(k)[..., 17:].any()
    k[6] = (10, 20, 2)                            # zero length: no limb
    assert not ref.skeleton(k)[..., 17:].any()


@pytest.mark.parametrize("hw", [(600, 300), (300, 600), (1, 1), (1000, 1400), (512, 512)])
def test_letterbox_matrix_and_plane(hw):
    h, w = hw
    m1 = ref.m1_of(h, w)
    s = m1[0]
    assert s == min(512 / w, 512 / h)
    assert abs(s * w / 2 + m1[2] - 256) < 1e-9 and abs(s * h / 2 + m1[5] - 256) < 1e-9   # centred
    img = np.full((h, w, 3), (10, 100, 200), np.uint8)
    out = ref.letterbox(img)
    assert out.shape == (512, 512, 4) and not out[..., 3].any()
    c0 = 0 if h == 1 else 256    # a 1 x 1 image: plane pixel (0, 0) samples its only pixel; (256, 256) lies half a source pixel past it
    for c, v in enumerate((10, 100, 200)):
        inside = np.float32((np.float32(v) / np.float32(255) - np.float32(ref.MEAN[c])) / np.float32(ref.STD[c]))
        zero = np.float32((np.float32(0) - np.float32(ref.MEAN[c])) / np.float32(ref.STD[c]))
        assert out[c0, c0, c] == inside and out[0, 0, c] in (zero, inside) and out[511, 511, c] in (zero, inside)
    sw = ref.letterbox(img, swap_rb=1)
    assert sw[c0, c0, 0] == np.float32((np.float32(200) / np.float32(255) - np.float32(ref.MEAN[0])) / np.float32(ref.STD[0]))


def test_letterbox_rounding_switch():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (37, 53, 3), np.uint8)
    a, b = ref.letterbox(img, round_u8=1), ref.letterbox(img, round_u8=0)
    assert not np.array_equal(a, b)
    v = a[..., 0] * np.float32(ref.STD[0]) + np.float32(ref.MEAN[0])
    assert np.allclose(v * 255, np.round(v * 255), atol=1e-3)


def test_reverse_warp_known_mask_and_box():
    logits = np.zeros((64, 64, 2), np.float32)
    logits[10:20, 5:15, 1] = 5.0
    m, box = ref.reverse_warp(logits, np.float32([1, 0, 0, 0, 1, 0]), 30, 40)
    assert m.shape == (30, 40) and m[10:20, 5:15].all() and m.sum() == 100
    assert list(box) == [5, 10, 15, 20]


def test_keypoint_json_reader_and_cli_parsing(tmp_path):
    from isegmi import cli
    from isegmi.pose2seg import read_person_keypoints
    d = {"images": [{"id": 7, "file_name": "a.png", "height": 20, "width": 30}],
         "annotations": [{"image_id": 7, "category_id": 1, "iscrowd": 0, "keypoints": list(range(51))},
                         {"image_id": 7, "category_id": 1, "iscrowd": 1, "keypoints": [0] * 51},
                         {"image_id": 7, "category_id": 1, "iscrowd": 0, "keypoints": [1] * 51}]}
    p = tmp_path / "kp.json"
    p.write_text(json.dumps(d))
    imgs, kp = read_person_keypoints(str(p))
    assert imgs[0]["file_name"] == "a.png" and kp[7].shape == (2, 17, 3) and kp[7][0, 1, 2] == 5 and kp[7][1].sum() == 51
    a = cli.build_parser().parse_args(["pose2seg_test", "--anno", str(p), "--image-root", str(tmp_path), "--batch-size", "4"])
    assert a.cmd == "pose2seg_test" and a.weights == "random" and a.batch_size == 4 and a.output == "segm.json"


def test_coco_records_from_masks():
    from isegmi.coco import rle_encode
    from isegmi.pose2seg import coco_results
    m = np.zeros((4, 3), np.uint8)
    m[1:3, 1] = 1
    r = coco_results(5, [m])
    assert r == [{"image_id": 5, "category_id": 1, "segmentation": rle_encode(m), "score": 1.0}]


def test_reference_weight_prep_is_torch_batchnorm_and_conv():
    """the restatement's own weight preparation (BN fold, KRSC, channel padding) against torch's BatchNorm2d / conv2d on one layer"""
    torch = pytest.importorskip("torch")
    from isegmi.weights import pose2seg_state_dict
    sd = pose2seg_state_dict(5, width=32, blocks=(1, 1, 1, 1), fpn_channels=32, seg_width=32, seg_blocks=(1, 1))
    p = ref.params_from_state_dict(sd, True)
    w, sc, sh = p["stages"][0][0]["conv2"]
    x = np.random.default_rng(0).standard_normal((1, 9, 9, 32)).astype(np.float32)
    got = ref.ora.conv2d(x, w, 1, 1, sc, sh)
    bn = torch.nn.BatchNorm2d(32).double().eval()
    nm = "backbone.layers.0.0.bn2"
    for a, k in ((bn.weight, "weight"), (bn.bias, "bias"), (bn.running_mean, "running_mean"), (bn.running_var, "running_var")):
        a.data = torch.tensor(sd[nm + "." + k], dtype=torch.float64)
    want = bn(torch.nn.functional.conv2d(torch.tensor(x.transpose(0, 3, 1, 2), dtype=torch.float64),
                                         torch.tensor(sd["backbone.layers.0.0.conv2.weight"], dtype=torch.float64), padding=1))
    np.testing.assert_allclose(got, want.detach().numpy().transpose(0, 2, 3, 1), rtol=1e-4, atol=1e-4)
    assert p["stem"][0].shape == (32, 7, 7, 4) and not p["stem"][0][..., 3].any()
    assert p["seg"]["conv1"][0].shape[3] == 96 and not p["seg"]["conv1"][0][..., 87:].any()

"""YOLOv3-SPP and YOLOv3-tiny on the CPU: the two .cfg files and the parser's refusals, the layer lists against the public files' sizes, the
.weights round trip, and -- with tests/yolo_variants_ref.py alone -- the pad fork of darknet's max-pool, its window rule and its NaN rule."""
import dataclasses
import os

import numpy as np
import pytest

import yolo_variants_ref as vr

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(name):
    return open(os.path.join(ROOT, "configs", name)).read()


# ---------------------------------------------------------------------------------------------------------------- .cfg
def test_cfg_files_parse_to_their_configs():
    from isegmi.config import parse_darknet_cfg, yolov3_cfg_text
    from isegmi.yolov3 import YoloV3Config
    assert parse_darknet_cfg(_cfg("yolov3.cfg")) == YoloV3Config()
    spp = parse_darknet_cfg(_cfg("yolov3-spp.cfg"))
    assert spp == YoloV3Config(variant="spp", height=608, width=608) and spp.strides == (32, 16, 8) and spp.pool_pad == "ignore"
    tiny = parse_darknet_cfg(_cfg("yolov3-tiny.cfg"))
    assert tiny == YoloV3Config.tiny() == YoloV3Config(variant="tiny", anchors=((10, 14), (23, 27), (37, 58), (81, 82), (135, 169), (344, 319)),
                                                       masks=((3, 4, 5), (0, 1, 2)))
    assert tiny.strides == (32, 16) and (tiny.height, tiny.width, tiny.classes) == (416, 416, 80)
    assert tiny.level_anchors().tolist() == vr.TINY_ANCHORS.tolist()
    assert parse_darknet_cfg(_cfg("yolov3-tiny.cfg"), pool_pad="zero", conf_thresh=0.1) == dataclasses.replace(tiny, pool_pad="zero", conf_thresh=0.1)
    # pjreddie's original second mask parses as well
    assert parse_darknet_cfg(_cfg("yolov3-tiny.cfg").replace("mask=0,1,2", "mask = 1,2,3")).masks == ((3, 4, 5), (1, 2, 3))
    for name, conv, pool, yolo in (("yolov3-spp.cfg", 76, 3, 3), ("yolov3-tiny.cfg", 13, 6, 2)):
        t = _cfg(name)
        assert (t.count("[convolutional]"), t.count("[maxpool]"), t.count("\n[yolo]")) == (conv, pool, yolo)
    assert _cfg("yolov3-spp.cfg").count("layers=-1,-3,-5,-6") == 1 and _cfg("yolov3-tiny.cfg").count("layers=-1, 8") == 1
    for c in (dataclasses.replace(spp, classes=20, height=416, width=320), dataclasses.replace(tiny, classes=3, height=64, width=96)):
        assert parse_darknet_cfg(yolov3_cfg_text(c)) == c


def test_refusals_name_the_section_or_key():
    from isegmi.config import parse_darknet_cfg
    from isegmi.yolov3 import YoloV3, YoloV3Config
    spp, tiny = _cfg("yolov3-spp.cfg"), _cfg("yolov3-tiny.cfg")
    with pytest.raises(ValueError, match=r"section 80 \[maxpool\].*'size': '7'.*YOLOv3-SPP"):
        parse_darknet_cfg(spp.replace("size=9", "size=7"))
    with pytest.raises(ValueError, match=r"3 \[yolo\] sections.*YOLOv3-tiny.*two"):
        parse_darknet_cfg(tiny + "\n[yolo]\nmask=0,1,2\nanchors=10,14, 23,27, 37,58, 81,82, 135,169, 344,319\nclasses=80\nnum=6\n")
    with pytest.raises(ValueError, match=r"section 11 \[maxpool\].*'stride': '2'.*YOLOv3-tiny"):
        parse_darknet_cfg(tiny.replace("size=2\nstride=1", "size=2\nstride=2"))
    with pytest.raises(ValueError, match=r"section 13 \[convolutional\].*YOLOv3-tiny"):
        parse_darknet_cfg(tiny.replace("filters=256\nactivation=leaky\n\n[convolutional]\nbatch_normalize=1\nsize=3\nstride=1\npad=1\nfilters=512",
                                       "filters=128\nactivation=leaky\n\n[convolutional]\nbatch_normalize=1\nsize=3\nstride=1\npad=1\nfilters=512"))
    with pytest.raises(ValueError, match="masks.*two"):
        YoloV3Config(variant="tiny").validate()
    with pytest.raises(ValueError, match="masks.*three"):
        dataclasses.replace(YoloV3Config.tiny(), variant="spp").validate()
    with pytest.raises(ValueError, match="variant"):
        YoloV3Config(variant="csp").validate()
    with pytest.raises(ValueError, match="pool_pad"):
        YoloV3Config(variant="spp", pool_pad="reflect").validate()
    for kw in (dict(fp16=True), dict(graph=True)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            YoloV3({}, cfg=YoloV3Config.tiny(), **kw)


def test_cli_takes_the_variants_and_the_pad_switch(monkeypatch):
    from isegmi.cli import build_parser, main, yolo_config
    tiny = os.path.join(ROOT, "configs", "yolov3-tiny.cfg")
    y = yolo_config(build_parser().parse_args(["yolo_detect", "--cfg", tiny, "--images", "D", "--img-size", "64", "96", "--pool-pad", "zero"]))
    assert (y.variant, y.pool_pad, y.height, y.width, y.strides) == ("tiny", "zero", 64, 96, (32, 16))
    y = yolo_config(build_parser().parse_args(["yolo_detect", "--cfg", os.path.join(ROOT, "configs", "yolov3-spp.cfg"), "--images", "D"]))
    assert (y.variant, y.pool_pad, y.height, y.width) == ("spp", "ignore", 608, 608)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["yolo_detect", "--cfg", tiny, "--images", "D", "--pool-pad", "reflect"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="world > 1"):
        main(["yolo_detect", "--cfg", tiny, "--images", "D"])


# ---------------------------------------------------------------------------------------------------------------- layer lists, .weights
def _file_bytes(layers):
    return 20 + 4 * sum(co * ci * k * k + (4 * co if bn else co) for _, bn, co, ci, k in layers)


def test_layer_lists_give_the_public_file_sizes():
    from isegmi.weights import yolo_layers, yolov3_layers
    spp, tiny, v3 = yolo_layers("spp", 80), yolo_layers("tiny", 80), yolo_layers("yolov3", 80)
    assert (len(spp), len(tiny), len(v3)) == (76, 13, 75) and v3 == yolov3_layers(80)
    assert _file_bytes(spp) == 252209544 and _file_bytes(tiny) == 35434956 and _file_bytes(v3) == 248007048
    names = [l[0] for l in spp]
    at = names.index("head.0.spp")
    assert names[at - 1: at + 2] == ["head.0.conv2", "head.0.spp", "head.0.conv3"] and spp[at][2:] == (512, 2048, 1)
    assert [l for l in spp if l[0] != "head.0.spp"] == v3
    assert [l[2] for l in tiny[:7]] == [16, 32, 64, 128, 256, 512, 1024] and [l[3] for l in tiny[:7]] == [3, 16, 32, 64, 128, 256, 512]
    assert [l[0] for l in tiny[7:]] == ["head.0.conv0", "head.0.conv1", "head.0.conv2", "head.1.route", "head.1.conv0", "head.1.conv1"]
    assert [l[1] is None for l in tiny[7:]] == [False, False, True, False, False, True] and tiny[11][2:] == (256, 384, 3)
    assert yolo_layers("tiny", 20)[9][2] == 75
    with pytest.raises(ValueError, match="variant"):
        yolo_layers("csp")


def test_tiny_weights_round_trip_and_the_wrong_topology(tmp_path):
    from isegmi.weights import load_darknet_weights, save_darknet_weights, yolo_layers
    from isegmi.yolov3 import YoloV3Config, yolov3_folded
    sd = vr.engine_weights("tiny")
    path = str(tmp_path / "yolov3-tiny.weights")
    save_darknet_weights(sd, path, variant="tiny")
    assert os.path.getsize(path) == 35434956
    back = load_darknet_weights(path, YoloV3Config.tiny())
    assert sorted(back) == sorted(sd) and all(np.array_equal(back[k], sd[k]) and back[k].dtype == np.float32 for k in sd)
    with pytest.raises(ValueError, match=r"too short.*backbone\.layers\.\d\.\d\.conv\d \((BN\.|weight)"):
        load_darknet_weights(path, YoloV3Config())
    with pytest.raises(ValueError, match=r"too short.*backbone\.layers\.\d\.\d\.conv\d \((BN\.|weight)"):
        load_darknet_weights(path, YoloV3Config(variant="spp"))
    with open(path, "ab") as f:
        f.write(b"\0\0\0\0")
    with pytest.raises(ValueError, match=r"too long.*head\.1\.conv1"):
        load_darknet_weights(path, YoloV3Config.tiny())
    folded = yolov3_folded(sd, YoloV3Config.tiny())
    assert list(folded) == [l[0] for l in yolo_layers("tiny")] and folded["backbone.conv0"][0].shape == (16, 3, 3, 3) and folded["head.1.conv1"][1] is None
    # the spp weights are the yolov3 ones of the same seed plus head.0.spp
    from isegmi.weights import yolov3_state_dict
    a, b = yolov3_state_dict(7), yolov3_state_dict(7, variant="spp")
    assert sorted(set(b) - set(a)) == ["head.0.spp.weight"] + ["head.0.spp_bn." + k for k in ("bias", "running_mean", "running_var", "weight")]
    assert all(np.array_equal(a[k], b[k]) for k in a) and b["head.0.spp.weight"].shape == (512, 2048, 1, 1)


# ---------------------------------------------------------------------------------------------------------------- the pool, with the reference alone
def test_pad_modes_differ_exactly_on_the_last_row_and_column():
    x = -(np.arange(36, dtype=F32).reshape(1, 3, 3, 4) + F32(1))   # all negative
    ign, zero = vr.maxpool_darknet(x, 2, 1), vr.maxpool_darknet(x, 2, 1, zero_pad=True)
    assert ign.shape == zero.shape == (1, 3, 3, 4)
    edge = np.zeros((3, 3), bool)
    edge[2, :] = edge[:, 2] = True
    assert ((ign != zero).all(-1)[0] == edge).all() and ((ign == zero).all(-1)[0] == ~edge).all()
    assert (zero[0][edge] == 0).all() and (ign < 0).all()
    # hand-derived: window (0, 0) holds pixels (0,0) (0,1) (1,0) (1,1), the largest (least negative) is pixel (0, 0); the corner window holds pixel (2, 2) alone
    assert np.array_equal(ign[0, 0, 0], x[0, 0, 0]) and np.array_equal(ign[0, 2, 2], x[0, 2, 2]) and np.array_equal(ign[0, 1, 2], x[0, 1, 2])
    # stride 2 on the odd map: (3 - 1) // 2 + 1 = 2 outputs, the second window starts at row 2 and sticks out
    s2 = vr.maxpool_darknet(x, 2, 2)
    assert s2.shape == (1, 2, 2, 4) and np.array_equal(s2[0, 1, 1], x[0, 2, 2]) and np.array_equal(s2[0, 0, 1], x[0, 0, 2])
    # wrong rules give other answers
    assert not np.array_equal(vr.maxpool_darknet(x, 2, 1, start_shift=1), ign)       # the window one to the top / left (padding on that side)
    assert np.array_equal(vr.maxpool_darknet(x, 2, 1, start_shift=1)[0, 1, 1], x[0, 0, 0])
    sym = vr.maxpool_darknet(x, 2, 1, symmetric=True)                                # nn.MaxPool2d(2, 1, padding=1)
    assert sym.shape == (1, 4, 4, 4) and not np.array_equal(sym[:, :3, :3], ign)   # another size; its top-left 3 x 3 is the shifted window's answer
    # odd sizes are centred: size 5 on a 1 x 1 map sees the one pixel; in zero mode the padding wins over a negative pixel
    one = x[:, :1, :1]
    assert np.array_equal(vr.maxpool_darknet(one, 5, 1), one) and (vr.maxpool_darknet(one, 5, 1, zero_pad=True) == 0).all()


def test_nan_rule_and_the_spp_order():
    x = np.random.default_rng(3).normal(0, 1, (1, 4, 5, 4)).astype(F32)
    x[0, 1, 2, 0] = np.nan; x[0, :, :, 1] = np.nan; x[0, 0, 0, 2] = np.inf; x[0, 3, 4, 3] = -np.inf
    for zp in (False, True):
        for size, stride in ((2, 1), (3, 2), (5, 1)):
            got = vr.maxpool_darknet(x, size, stride, zp)
            assert not np.isnan(got).any()
            if not zp:
                assert (got[..., 1] == -np.inf).all()   # the all-NaN channel
            # the largest non-NaN tap: the same as a pool of the input with every NaN replaced by -inf
            assert np.array_equal(got, vr.maxpool_darknet(np.where(np.isnan(x), F32(-np.inf), x), size, stride, zp))
    assert vr.maxpool_darknet(x, 3, 1)[0, 1, 2, 0] == np.nanmax(x[0, 0:3, 1:4, 0])
    assert vr.maxpool_darknet(x, 5, 1)[0, 0, 0, 2] == np.inf
    # zero mode, all-NaN channel: 0 exactly where the window leaves the map (size 3, stride 1: the border ring), -inf inside
    z = vr.maxpool_darknet(x, 3, 1, zero_pad=True)[0, :, :, 1]
    ring = np.ones((4, 5), bool)
    ring[1:-1, 1:-1] = False
    assert (z[ring] == 0).all() and (z[~ring] == -np.inf).all()
    s = vr.spp_concat(x[..., :4])
    assert s.shape == (1, 4, 5, 16) and np.array_equal(s[..., 12:], x, equal_nan=True)
    assert np.array_equal(s[..., 8:12], vr.maxpool_darknet(x, 5, 1)) and np.array_equal(s[..., :4], vr.maxpool_darknet(x, 13, 1))
    # the two identities the device kernel rests on: the cascade with padding ignored, and zero mode = the ignore-mode value with one +0.0 folded in
    # exactly where the output's own window leaves the map
    neg = -np.abs(np.random.default_rng(4).normal(0, 1, (1, 15, 14, 4)).astype(F32)) - F32(0.1)
    mp = lambda a, k, zp=False: vr.maxpool_darknet(a, k, 1, zp)
    assert np.array_equal(mp(mp(neg, 5), 5), mp(neg, 9)) and np.array_equal(mp(mp(neg, 9), 5), mp(neg, 13))
    for k in (5, 9, 13):
        r = k // 2
        out = np.ones((15, 14), bool)
        out[r:15 - r, r:14 - r] = False
        assert np.array_equal(np.where(out[None, :, :, None], np.maximum(mp(neg, k), 0), mp(neg, k)), mp(neg, k, True)) and (~out).any() and out.any()


@pytest.mark.parametrize("canvas", vr.ENGINE_CANVASES)
def test_engine_seeds_give_every_level_candidates(canvas):
    """In the reference alone: at ENGINE_CONF every level of both variants has a candidate on every image, and tiny's heads differ between the pad modes."""
    for variant in ("spp", "tiny"):
        ref, dets = vr.engine_reference(variant, *canvas)
        strides = (32, 16, 8) if variant == "spp" else (32, 16)
        assert [h.shape[1:] for h in ref.feats["heads"]] == [(canvas[0] // s, canvas[1] // s, 255) for s in strides]
        assert (ref.feats["total"] >= 1).all() and all(len(d["score"]) >= 1 for d in dets)
    a, b = vr.engine_reference("tiny", *canvas)[0].feats["heads"], vr.engine_reference("tiny", *canvas, zero_pad=True)[0].feats["heads"]
    assert all(not np.array_equal(x, y) for x, y in zip(a, b))

"""Second opinion on Pose2Seg without a GPU (CPU only).

Stage by stage, the restatement tests/pose2seg_ref.py (which the GPU kernels match bit for bit) against the independent fp64 restatement
tests/pose2seg_fp64.py, under the error bounds derived there: a misconception the kernels and pose2seg_ref.py share (sigma, the limb
table, the matrix order of Mmask, the mask threshold, the limb window) fails here.

Then the whole forward a second time as a torch `nn.Module` tree, NCHW and fp64, named like weights.pose2seg_state_dict and loaded with
`load_state_dict(strict=True)`: torch's conv, BatchNorm (eval), max-pool, `F.interpolate` and `affine_grid` + `grid_sample`, the fit,
skeleton and mask sampling from pose2seg_fp64.py.  P2, the RoI tensor and the logits must match pose2seg_ref.forward within 1e-4 of each
tensor's largest magnitude (the two sides sum in different orders and precisions); masks and boxes must match outside the band where the
foreground probability is within that logit tolerance of 0.5.  Narrow widths, blocks (2, 2, 2, 2) and seg_blocks (3, 2), so non-first
blocks and projections are included; both cat_skeleton and both fpn_upsample values.
"""
import numpy as np
import pytest

import pose2seg_fp64 as f64
import pose2seg_ref as ref
from isegmi.weights import pose_templates

torch = pytest.importorskip("torch")
nn = torch.nn
F = torch.nn.functional


# ---------------------------------------------------------------------------------------------------- stages: pose2seg_ref vs fp64
@pytest.mark.parametrize("swap_rb,round_u8", [(0, 1), (1, 0), (0, 0)])
def test_ref_letterbox_within_fp64_bounds(swap_rb, round_u8):
    rng = np.random.default_rng(40 + swap_rb)
    amb = f64.Ambiguity()
    for hw in ((300, 200), (97, 131), (640, 480), (1, 1), (2, 700)):
        img = f64.smooth_image(rng, *hw)
        f64.check_letterbox(ref.letterbox(img, swap_rb, round_u8), img, swap_rb, round_u8, amb)
    if round_u8:
        amb.check()


def _fit_all(k, hw_of, tp, align_corners):
    """ref.fit of every person, checked against fp64; returns the template indices"""
    ts, decided = [], 0
    for r in range(len(k)):
        m1 = f64.m1_matrix(*hw_of[r])
        f = ref.fit(k[r], list(m1[:2].ravel()), tp, align_corners)
        w = f64.fit(k[r], m1, tp, align_corners)
        decided += f64.check_fit(f["m3"], f["G"], f["mmask"], f["kalign"], f["t"], w)
        ts.append(f["t"])
        assert np.all(np.isfinite(f["m3"])) and np.all(np.isfinite(f["G"])), r
    assert decided >= len(k) - 1
    return ts


@pytest.mark.parametrize("align_corners", [0, 1])
@pytest.mark.parametrize("T", [1, 3, 64])
def test_ref_fit_within_fp64_bounds(align_corners, T):
    rng = np.random.default_rng(50 + T)
    hws = [(480, 640), (300, 200)]
    k = np.concatenate([f64.edge_persons(rng, *hws[0]), f64.persons(rng, 6, *hws[1], invisible=0.4)])
    hw_of = [hws[0]] * (len(k) - 6) + [hws[1]] * 6
    tp = pose_templates() if T == 3 else f64.random_templates(rng, T)
    if T == 3:   # one exact template image: the fit recovers it
        m1 = f64.m1_matrix(*hws[0])
        A = np.array([[0.8, 0.12, -30.0], [-0.07, 0.95, -12.5], [0, 0, 1]])
        ki = np.linalg.solve(A @ f64.M2 @ m1, np.vstack([tp[1, :, 0], tp[1, :, 1], np.ones(17)]))
        k[0] = np.stack([ki[0], ki[1], np.full(17, 2.0)], 1).astype(np.float32)
    ts = _fit_all(k, hw_of, tp, align_corners)
    assert -1 in ts and max(ts) >= 0


def test_nonfinite_keypoints_are_invisible():
    """a NaN / +-inf coordinate counts as not visible: the fit and the fallback box skip it and kalign carries v = 0 for it"""
    rng = np.random.default_rng(3)
    m1 = f64.m1_matrix(480, 640)
    tp = pose_templates()
    k = f64.persons(rng, 1, 480, 640, invisible=0)[0]
    clean = ref.fit(k, list(m1[:2].ravel()), tp)
    k2 = k.copy(); k2[0, 0] = np.nan; k2[5, 1] = np.inf
    drop = k.copy(); drop[[0, 5], 2] = 0
    f, g = ref.fit(k2, list(m1[:2].ravel()), tp), ref.fit(drop, list(m1[:2].ravel()), tp)
    assert f["t"] == g["t"] >= 0 and np.array_equal(f["m3"], g["m3"]) and np.array_equal(f["G"], g["G"]) and f["err"] == g["err"]
    assert f["kalign"][0, 2] == 0 and f["kalign"][5, 2] == 0 and clean["kalign"][0, 2] == 2
    fb = k.copy(); fb[2:, 2] = 0; fb[0, 0] = np.nan                     # fallback: NaN on the first visible keypoint, one finite point left
    f = ref.fit(fb, list(m1[:2].ravel()), tp)
    assert f["t"] == -1 and np.all(np.isfinite(f["m3"])) and f["m3"][0] == 8.0
    assert f64.check_fit(f["m3"], f["G"], f["mmask"], f["kalign"], f["t"], f64.fit(fb, m1, tp))


@pytest.mark.parametrize("align_corners", [0, 1])
def test_ref_align_within_fp64_bounds(align_corners):
    rng = np.random.default_rng(60 + align_corners)
    feat = rng.standard_normal((128, 128, 8)).astype(np.float32)
    for H in ([0.9, 0.15, -20.0, -0.1, 1.1, -15.0], [0.5, 0, 0, 0, 0.5, 0], [1.3, 0.2, -5.0, -0.1, 1.2, 90.0], [2.0, -0.3, 10.0, 0.4, 1.7, -60.0]):
        H = np.vstack([np.reshape(H, (2, 3)), [0, 0, 1]])
        G32 = np.array(ref.align_matrix(list(H.ravel()), align_corners)[:6]).astype(np.float32)
        f64.check_align(ref.affine_align(feat, G32), feat, H, align_corners)


def test_ref_skeleton_within_fp64_bounds():
    rng = np.random.default_rng(70)
    amb = f64.Ambiguity()
    kal = np.zeros((6, 17, 3), np.float32)
    kal[..., :2] = rng.uniform(-10, 74, (6, 17, 2))
    kal[..., 2] = np.where(rng.uniform(size=(6, 17)) < 0.2, 0, 2)
    kal[1, 5, :2] = kal[1, 6, :2] = (20.0, 30.0)                    # zero-length limb
    kal[1, 7, :2] = (20.0, 50.0)                                    # axis-aligned limbs
    kal[1, 9, :2] = (44.0, 50.0)
    kal[2, :, :2] = rng.uniform(20, 44, (17, 2))
    for k in kal:
        f64.check_skeleton(ref.skeleton(k), k, amb)
    amb.check()
    assert amb.total > 0 and any(ref.skeleton(k)[..., 17:].any() for k in kal)


def test_ref_masks_within_fp64_bounds():
    rng = np.random.default_rng(80)
    amb = f64.Ambiguity()
    n_on = []
    for i, (h, w) in enumerate(((50, 70), (90, 40), (333, 500), (1, 1))):
        lg = np.cumsum(np.cumsum(rng.standard_normal((64, 64, 2)), 0), 1).astype(np.float32) * 0.05   # smooth logits
        s = rng.uniform(0.1, 2.5)
        mm = np.float32([s, rng.uniform(-0.2, 0.2), rng.uniform(-20, 30), rng.uniform(-0.2, 0.2), s, rng.uniform(-20, 30)])
        m, b = ref.reverse_warp(lg, mm, h, w)
        f64.check_mask(m, b, lg, mm, h, w, amb)
        n_on.append(m.mean())
    amb.check()
    assert max(n_on) > 0 and min(n_on[:3]) < 1
    eq = np.full((64, 64, 2), 0.75, np.float32)                     # p = 0.5 exactly: not foreground
    m, b = ref.reverse_warp(eq, np.float32([0.5, 0, 3, 0, 0.5, 4]), 60, 60)
    assert not m.any() and not b.any()


# ---------------------------------------------------------------------------------------------------- the torch composition
class Bottleneck(nn.Module):
    """torchvision's: stride on conv2, projection = downsample.{0: conv, 1: BN}"""

    def __init__(self, cin, planes, stride, proj):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(cin, planes, 1, bias=False), nn.BatchNorm2d(planes)
        self.conv2, self.bn2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False), nn.BatchNorm2d(planes)
        self.conv3, self.bn3 = nn.Conv2d(planes, planes * 4, 1, bias=False), nn.BatchNorm2d(planes * 4)
        self.downsample = nn.Sequential(nn.Conv2d(cin, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4)) if proj else None

    def forward(self, x):
        t = F.relu(self.bn1(self.conv1(x)))
        t = F.relu(self.bn2(self.conv2(t)))
        t = self.bn3(self.conv3(t))
        return F.relu(t + (x if self.downsample is None else self.downsample(x)))


class Backbone(nn.Module):
    def __init__(self, width, blocks):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(3, width, 7, 2, 3, bias=False), nn.BatchNorm2d(width)
        layers, cin = [], width
        for li, nb in enumerate(blocks):
            planes = width << li
            layers.append(nn.Sequential(*[Bottleneck(cin if b == 0 else planes * 4, planes, 2 if (li > 0 and b == 0) else 1, b == 0)
                                          for b in range(nb)]))
            cin = planes * 4
        self.layers = nn.ModuleList(layers)

    def forward(self, x):
        x = F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        out = []
        for layer in self.layers:
            x = layer(x)
            out.append(x)
        return out


class FPN(nn.Module):
    def __init__(self, width, C, upsample):
        super().__init__()
        for l in (2, 3, 4, 5):
            setattr(self, "lateral%d" % l, nn.Conv2d((width * 4) << (l - 2), C, 1))
            setattr(self, "output%d" % l, nn.Conv2d(C, C, 3, 1, 1))
        self.upsample = upsample

    def forward(self, c):
        inner = self.lateral5(c[3])
        for l in (4, 3, 2):
            lat = getattr(self, "lateral%d" % l)(c[l - 2])
            if self.upsample == "nearest":
                up = F.interpolate(inner, scale_factor=2, mode="nearest")
            else:
                up = F.interpolate(inner, size=lat.shape[-2:], mode="bilinear", align_corners=False)
            inner = lat + up
        return self.output2(inner)


class SegNet(nn.Module):
    def __init__(self, cin, width, blocks):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(cin, width, 7, 2, 3, bias=False), nn.BatchNorm2d(width)
        stages, c = [], width
        for nb in blocks:
            stages.append(nn.Sequential(*[Bottleneck(c if b == 0 else width * 4, width, 1, b == 0 and c != width * 4) for b in range(nb)]))
            c = width * 4
        self.stage1, self.stage2 = stages
        self.conv_out = nn.Conv2d(width * 4, 2, 1)

    def forward(self, x):
        x = self.stage1(F.relu(self.bn1(self.conv1(x))))
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        return self.conv_out(self.stage2(x))


class Pose2SegNet(nn.Module):
    def __init__(self, sd, fpn_upsample):
        super().__init__()
        width = sd["backbone.conv1.weight"].shape[0]
        nblk = lambda pre: len({k[len(pre):].split(".")[0] for k in sd if k.startswith(pre)})
        C = sd["fpn.output2.weight"].shape[0]
        self.backbone = Backbone(width, [nblk("backbone.layers.%d." % l) for l in range(4)])
        self.fpn = FPN(width, C, fpn_upsample)
        self.segnet = SegNet(sd["segnet.conv1.weight"].shape[1], sd["segnet.conv1.weight"].shape[0], [nblk("segnet.stage1."), nblk("segnet.stage2.")])
        self.register_buffer("pose_templates", torch.zeros(sd["pose_templates"].shape))
        t = {k: torch.tensor(np.asarray(v)) for k, v in sd.items()}
        for k in self.state_dict():
            if k.endswith("num_batches_tracked"):
                t[k] = torch.tensor(0)
        self.double().load_state_dict(t, strict=True)
        self.eval()


def _weights(cat_skeleton, seed=31):
    from isegmi.weights import pose2seg_state_dict
    return pose2seg_state_dict(seed, cat_skeleton=cat_skeleton, width=16, blocks=(2, 2, 2, 2), fpn_channels=32, seg_width=16, seg_blocks=(3, 2))


def _torch_forward(net, images, kpts, cfg):
    x = np.stack([f64.normalise(np.clip(np.floor(f64.letterbox(im, cfg.swap_rb)[0] + 0.5), 0, 255) if cfg.warp_round_u8
                                else f64.letterbox(im, cfg.swap_rb)[0]) for im in images])
    with torch.no_grad():
        p2 = net.fpn(net.backbone(torch.tensor(x.transpose(0, 3, 1, 2))))
        tp = net.pose_templates.numpy()
        A = np.array([[2 / 128, 0, -1], [0, 2 / 128, -1], [0, 0, 1]])
        rois, fits = [], []
        for n, (im, kp) in enumerate(zip(images, kpts)):
            for k in kp:
                f = f64.fit(k, f64.m1_matrix(*im.shape[:2]), tp, cfg.align_corners)
                theta = np.linalg.inv(A @ f["H"] @ np.linalg.inv(A))[:2]
                grid = F.affine_grid(torch.tensor(theta[None]), (1, p2.shape[1], 128, 128), align_corners=bool(cfg.align_corners))
                r = F.grid_sample(p2[n:n + 1], grid, mode="bilinear", padding_mode="zeros", align_corners=bool(cfg.align_corners))[..., :64, :64]
                if cfg.cat_skeleton:
                    kal = f["kalign"].astype(np.float32)         # the contract hands the skeleton fp32 align-frame keypoints
                    r = torch.cat([r, torch.tensor(f64.skeleton(kal).transpose(2, 0, 1)[None])], 1)
                rois.append(r); fits.append(f)
        roi = torch.cat(rois)
        logits = net.segnet(roi)
    return p2, roi, logits, fits


def _close(got_nchw, want_nhwc, name, tol=1e-4):
    g = got_nchw.permute(0, 2, 3, 1).numpy()
    w = np.asarray(want_nhwc, np.float64)
    assert g.shape == w.shape, (name, g.shape, w.shape)
    err = np.abs(g - w).max() / max(1e-6, np.abs(w).max())
    assert err < tol, (name, err)


@pytest.mark.parametrize("cat_skeleton,fpn_upsample,align_corners", [(1, "nearest", 0), (1, "bilinear", 1), (0, "bilinear", 0), (0, "nearest", 1)])
def test_torch_composition_matches_ref_forward(cat_skeleton, fpn_upsample, align_corners):
    from isegmi.pose2seg import Pose2SegConfig
    cfg = Pose2SegConfig(cat_skeleton=cat_skeleton, fpn_upsample=fpn_upsample, align_corners=align_corners)
    sd = _weights(bool(cat_skeleton))
    rng = np.random.default_rng(90)
    # letterbox scales that are powers of two: every sample lands on a pixel or a half, so the u8 rounding is exact on both sides
    images = [rng.integers(0, 256, hw + (3,), np.uint8) for hw in ((256, 128), (128, 512))]
    kpts = [f64.persons(rng, 3, 256, 128), f64.persons(rng, 2, 128, 512)]
    kpts[0][2, :, 2] = 0                                          # the fallback
    net = Pose2SegNet(sd, fpn_upsample)
    # shift the foreground bias so the masks are neither empty nor full
    _, _, lg, _ = _torch_forward(net, images, kpts, cfg)
    sd["segnet.conv_out.bias"] = sd["segnet.conv_out.bias"].copy()
    sd["segnet.conv_out.bias"][1] -= float(np.median((lg[:, 1] - lg[:, 0]).numpy()))
    net = Pose2SegNet(sd, fpn_upsample)
    p2, roi, logits, fits = _torch_forward(net, images, kpts, cfg)
    want = ref.forward(sd, images, kpts, cfg)
    croi = roi.shape[1]
    _close(p2, want["p2"], "p2")
    _close(roi, want["roi"][..., :croi], "roi")
    assert not want["roi"][..., croi:].any()
    _close(logits, want["logits"], "logits")
    assert [f["t"] for f in fits] == [f["t"] for f in want["fits"]] and -1 in [f["t"] for f in fits]
    lg = logits.permute(0, 2, 3, 1).numpy()
    extra = 0.25 * 2 * 1e-4 * np.abs(want["logits"]).max()      # |dp| <= |d(l1 - l0)| / 4
    amb, r, fg = f64.Ambiguity(), 0, []
    for n, im in enumerate(images):
        for k in range(len(kpts[n])):
            f64.check_mask(want["masks"][n][k], want["boxes"][n][k], lg[r], fits[r]["Mmask"], *im.shape[:2], amb, extra)
            fg.append(want["masks"][n][k].mean())
            r += 1
    amb.check()
    assert max(fg) > 0 and min(fg) < 1
    p = f64.softmax_fg(lg)
    assert 0.1 < (p > 0.5).mean() < 0.9

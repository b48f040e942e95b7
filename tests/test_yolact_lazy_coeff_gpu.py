"""Yolact fp32 `lazy_coeffs`: the forward runs the loc|conf rows of the fused prediction head only and the mask coefficients of the kept detections are
computed after the final top-k (csrc/yolact_coeff.hip).  Nothing may change: the operator must return the head convolution's own bytes, and an engine
with lazy_coeffs 1 must give the bytes of lazy_coeffs 0 in every launch form -- including a `headcat` fetched in full."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEVELS = ((5, 5), (3, 3), (2, 2), (1, 1), (1, 1))   # corners, edges, and the 1x1 maps where eight of nine taps are padding
CIN = 256
_ref_cache = {}


def _op_case(A, kind):
    """inputs, the row list and the expected rows of one operator case; computed once per (A, kind) and never modified"""
    key = (A, kind)
    if key in _ref_cache:
        return _ref_cache[key]
    from isegmi import _ffi
    from oracle import ora
    rng = np.random.default_rng(1000 * A + len(kind))
    N, cout = 3, 117 * A
    if kind == "int":   # exact small integers: every partial sum is an integer below 2^24
        feats = [rng.integers(-3, 4, (N, h, w, CIN)).astype(np.float32) for h, w in LEVELS]
        wt = rng.integers(-3, 4, (cout, 3, 3, CIN)).astype(np.float32)
        bias = rng.integers(-8, 9, cout).astype(np.float32)
    else:
        feats = [rng.standard_normal((N, h, w, CIN)).astype(np.float32) for h, w in LEVELS]
        wt = (rng.standard_normal((cout, 3, 3, CIN)) * 0.05).astype(np.float32)
        bias = rng.standard_normal(cout).astype(np.float32)
    # every pixel of every level with every anchor, then duplicates
    base = [(l, ho, wo, a) for l, (h, w) in enumerate(LEVELS) for ho in range(h) for wo in range(w) for a in range(A)]
    base += base[:5] + base[-2:]
    max_det = len(base)
    rows = np.array([[(n,) + r for r in base] for n in range(N)], np.int32)
    counts = np.array([0, 1, max_det], np.int32)
    full = [_ffi.conv2d(f, wt, pad=1, shift=bias) for f in feats]          # the head convolution through the conv operator
    full_ora = [ora.conv2d(f, wt, pad=1, shift=bias) for f in feats]
    pick = lambda outs: np.array([[outs[l][n, ho, wo, 85 * A + 32 * a:85 * A + 32 * a + 32] for (l, ho, wo, a) in base] for n in range(N)], np.float32)
    case = dict(feats=feats, w=wt, bias=bias, rows=rows, counts=counts, want=pick(full), want_ora=pick(full_ora))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _ref_cache[key] = case
    return case


@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("A", [3, 9])
def test_coeff_rows_are_the_head_convolutions_bytes(ffi, A, kind):
    c = _op_case(A, kind)
    assert np.array_equal(c["want"].view(np.uint32), c["want_ora"].view(np.uint32))   # conv operator == oracle at these pixels and columns
    got = ffi.yolact_coeff_rows(c["feats"], c["w"], c["bias"], A, c["rows"], c["counts"], row0=85 * A)
    bits, want = got.view(np.uint32), c["want"].view(np.uint32)
    for n, cnt in enumerate(c["counts"]):
        assert np.array_equal(bits[n, :cnt], want[n, :cnt]), ("image", n)
        assert (bits[n, cnt:] == 0xFFFFFFFF).all(), ("slots past the count were written", n)   # the 0xFF sentinel of the wrapper
    assert c["counts"][2] == got.shape[1] > 40 * A


def test_coeff_rows_ignores_marked_and_out_of_range_rows(ffi):
    """a negative level marks an invalid slot; rows that point outside their level, image or anchor range are dropped, not read"""
    c = _op_case(3, "int")
    rows = np.array(c["rows"][:, :8])
    rows[2, 0] = (-1, -1, -1, -1, -1)
    rows[2, 1] = (2, 0, 5, 0, 0)     # ho past the 5 x 5 level
    rows[2, 2] = (2, 1, 0, 3, 0)     # wo past the 3 x 3 level
    rows[2, 3] = (2, 0, 0, 0, 3)     # anchor == A
    rows[2, 4] = (3, 0, 0, 0, 0)     # image == N
    rows[2, 5] = (2, 5, 0, 0, 0)     # level == nlevels
    got = ffi.yolact_coeff_rows(c["feats"], c["w"], c["bias"], 3, rows, np.array([0, 1, 8], np.int32), row0=255).view(np.uint32)
    assert (got[2, :6] == 0xFFFFFFFF).all()
    assert np.array_equal(got[2, 6:8], c["want"][2, 6:8].view(np.uint32)) and np.array_equal(got[1, :1], c["want"][1, :1].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------- engine
KEYS = ("det.count", "det.score", "det.box", "det.class", "det.coeff", "det.prior")


@pytest.fixture(scope="module")
def sd():
    from isegmi.weights import yolact_state_dict
    return yolact_state_dict(1234)


@pytest.fixture(scope="module")
def sd_plus():
    from isegmi.weights import yolact_state_dict
    from isegmi.yolact import YolactConfig
    cfg = YolactConfig.plus_resnet50()
    return cfg, yolact_state_dict(77, depth=cfg.depth, num_priors=9, dcn_layers=cfg.dcn_layers, dcn_interval=cfg.dcn_interval)


def _images(seed, n, size=200):
    from isegmi.yolact import fast_base_transform
    rng = np.random.default_rng(seed)
    return fast_base_transform(rng.uniform(0, 255, (n, size, size, 3)).astype(np.float32))


def _net(sd, n, params, cfg=None):
    from isegmi.yolact import Yolact
    net = Yolact(sd, max_batch=n, input_size=200) if cfg is None else Yolact(sd, cfg=cfg, max_batch=n, input_size=200)
    for k, v in params.items():
        net.set_param(k, float(v))
    return net


def _step(net, x, masks=True):
    n = net.upload(x)
    net.forward_device(n)
    if masks:
        net.postprocess_device(200, 200)
    net.sync()
    r = {k: net.fetch(k, n) for k in KEYS}
    if masks:
        r["masks"] = net.fetch("det.masks", n)
    return r


def _same(a, b):
    """every det.* array whole (slots past the count are zero-filled by the gather), the masks below the counts"""
    for k in KEYS:
        assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k], b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]), k
    if "masks" in a:
        for n, c in enumerate(a["det.count"]):
            assert np.array_equal(a["masks"][n, :c], b["masks"][n, :c]), ("masks", n)


VARIANTS = {"default": {}, "per_level": dict(conv_groups=0), "one_stream": dict(multi_stream=0), "per_level_one_stream": dict(conv_groups=0, multi_stream=0)}


@pytest.mark.parametrize("N", [2, 1])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_lazy_engine_equals_eager_engine(ffi, sd, variant, N):
    """lazy first, on a fresh engine whose headcat has never held a coefficient; twice, so that the second forward runs against the first one's tail"""
    x = _images(40 + N, N)
    net = _net(sd, N, dict(VARIANTS[variant], lazy_coeffs=1))
    lazy = [_step(net, x) for _ in range(2)]
    assert net.fetch("ws.coeff_sel", N).shape == (N, 100, 32)
    net.close()
    net = _net(sd, N, dict(VARIANTS[variant], lazy_coeffs=0))
    eager = _step(net, x)
    net.close()
    assert int(eager["det.count"].sum()) > 0 and np.abs(eager["det.coeff"]).max() > 0
    _same(lazy[0], eager)
    _same(lazy[1], eager)


@pytest.mark.parametrize("N", [2, 1])
def test_lazy_engine_yolact_plus_nine_anchors(ffi, sd_plus, N):
    cfg, sdp = sd_plus
    x = _images(50 + N, N)
    res = []
    for lazy in (1, 0):
        net = _net(sdp, N, dict(lazy_coeffs=lazy), cfg)
        res.append(_step(net, x))
        net.close()
    assert int(res[1]["det.count"].sum()) > 0
    _same(res[0], res[1])


@pytest.mark.parametrize("N", [2, 1])
@pytest.mark.parametrize("variant", ["default", "per_level"])
def test_headcat_fetched_after_a_lazy_forward_is_complete(ffi, sd, variant, N):
    """forward -> fetch headcat -> forward -> fetch: both fetches hold all 117 A columns of the eager run, and the fetch disturbs no detection"""
    xa, xb = _images(60 + N, N), _images(70 + N, N)
    net = _net(sd, N, dict(VARIANTS[variant], lazy_coeffs=0))
    want = []
    for x in (xa, xb):
        r = _step(net, x)
        r["headcat"] = net.fetch("headcat", N)
        want.append(r)
    net.close()
    assert not np.array_equal(want[0]["headcat"], want[1]["headcat"])
    net = _net(sd, N, dict(VARIANTS[variant], lazy_coeffs=1))
    for x, w in zip((xa, xb), want):
        n = net.upload(x)
        net.forward_device(n)
        net.sync()
        before = {k: net.fetch(k, n) for k in KEYS}
        hc = net.fetch("headcat", n)
        assert np.array_equal(hc.view(np.uint32), w["headcat"].view(np.uint32))
        assert np.array_equal(net.fetch("headcat", n).view(np.uint32), hc.view(np.uint32))   # a second fetch: nothing to fill, same bytes
        net.postprocess_device(200, 200); net.sync()
        after = {k: net.fetch(k, n) for k in KEYS}
        after["masks"] = net.fetch("det.masks", n)
        for k in KEYS:
            assert np.array_equal(before[k], after[k]), ("the fetch changed", k)
        _same(after, w)
    net.close()


def test_two_lazy_forwards_without_a_fetch_read_no_stale_column(ffi, sd):
    xa, xb = _images(81, 2), _images(82, 2)
    net = _net(sd, 2, dict(lazy_coeffs=1))
    net.upload(xa)
    net.input_buffer(1).upload(xb)
    net.forward_device(2, slot=0)   # back to back from the two input slots: no sync and no fetch in between
    net.forward_device(2, slot=1)
    net.postprocess_device(200, 200); net.sync()
    got = {k: net.fetch(k, 2) for k in KEYS}
    got["masks"] = net.fetch("det.masks", 2)
    net.close()
    net = _net(sd, 2, dict(lazy_coeffs=0))
    first, want = _step(net, xa), _step(net, xb)
    net.close()
    assert not np.array_equal(first["det.coeff"], want["det.coeff"])
    _same(got, want)


def test_an_image_without_detections(ffi, sd):
    """a constant image next to a random one, nms_conf_thresh raised (set_param) to where one of the two keeps nothing"""
    x = np.array(_images(90, 2))
    x[1] = x[1].mean()
    net = _net(sd, 2, dict(lazy_coeffs=0))
    r = _step(net, x, masks=False)
    top = [float(r["det.score"][n, :r["det.count"][n]].max()) if r["det.count"][n] else 0.0 for n in range(2)]
    assert top[0] != top[1]
    thr = 0.5 * (top[0] + top[1])   # between the two images' best scores: fast-NMS keeps a class's best box, so the other image keeps >= 1
    net.set_param("nms_conf_thresh", thr)
    eager = _step(net, x)
    net.close()
    assert sorted(int(c > 0) for c in eager["det.count"]) == [0, 1]
    net = _net(sd, 2, dict(lazy_coeffs=1, nms_conf_thresh=thr))
    lazy = _step(net, x)
    net.close()
    _same(lazy, eager)
    empty = int(np.argmin(eager["det.count"]))
    assert not lazy["det.coeff"][empty].any() and (lazy["det.class"][empty] == -1).all()


def test_default_is_by_batch_size_and_fp16_keeps_the_full_head(ffi, sd):
    """-1: off at the latency batches, on from three images; lazy_coeffs 1 on an fp16 engine changes nothing (the fp16 mode keeps the full head)"""
    from isegmi.yolact import Yolact
    for n, on in ((2, False), (3, True)):
        net = _net(sd, n, {})
        r = _step(net, _images(95, n), masks=False)
        names_ok = True
        try:
            net.fetch("ws.coeff_sel", n)
        except Exception:
            names_ok = False
        net.close()
        assert names_ok == on, (n, names_ok)
        if on:
            net = _net(sd, n, dict(lazy_coeffs=0))
            _same(r, _step(net, _images(95, n), masks=False))
            net.close()
    x = _images(96, 1)
    res = []
    for lazy in (1, 0):
        net = Yolact(sd, max_batch=1, input_size=200, fp16=True)
        net.set_param("lazy_coeffs", float(lazy))
        res.append(_step(net, x, masks=False))
        net.close()
    _same(res[0], res[1])

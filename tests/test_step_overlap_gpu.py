"""Two backbone lanes of the Yolact fp32 engine (engine parameter `step_overlap`, csrc/engine.cpp): consecutive forwards alternate between two
lanes -- a main stream with its side streams and its own backbone / FPN buffers -- so that step i + 1's backbone overlaps step i's.  The same
kernels run on the same operands, only stream and buffer differ: every result must equal, bit for bit, what one lane gives and what an isolated
forward + sync gives, however the steps are queued.

How a queued step's results are kept: nothing may wait on the host between the steps, and det.* / proto / the mask planes exist once, so every
step snapshots them ON ITS RESULTS STREAM -- isegmi_yolact_pack_records (count, box, score, class, coeff, proto) into a device block of its own,
isegmi_engine_download_async of det.prior / det.box_int / det.masks into pinned blocks of its own -- and leaves a completion mark; the host
reads a step's snapshot after waiting for that step's mark."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE, HI, WI, K, MD = 200, 150, 180, 100, 32   # network input; raw uint8 image size (the device front end resizes); detections, mask dim
FIELDS = ("count", "box", "score", "cls", "coeff", "proto", "prior", "box_int", "masks")


def lane_layout(ffi, net):
    out = (C.c_int32 * 18)()
    ffi.check(ffi.lib().isegmi_engine_lane_layout(net._h, out, 18))
    return [int(v) for v in out]


def isolated(net, batch):
    """forward_device + sync of one batch, results fetched from the engine's buffers"""
    n = net.upload_u8(batch)
    net.forward_device(n)
    net.postprocess_device(HI, WI)
    net.sync()
    r = {"count": net.fetch("det.count", n), "box": net.fetch("det.box", n), "score": net.fetch("det.score", n), "cls": net.fetch("det.class", n),
         "coeff": net.fetch("det.coeff", n), "proto": net.fetch("proto", n), "prior": net.fetch("det.prior", n),
         "box_int": net.fetch("det.box_int", n), "masks": net.fetch("det.masks", n)}
    assert int(r["count"].sum()) > 0, "no detections: an empty result would compare nothing"
    return r


class Queue:
    """Steps queued back to back; see the module docstring for how their results are kept."""
    proto_hw = None   # (PH, PW) of the prototypes, set by the rig from a first forward

    def __init__(self, ffi, net):
        self.ffi, self.net, self.steps = ffi, net, []

    def _ptr(self, name):
        p = C.c_void_p()
        self.ffi.check(self.ffi.lib().isegmi_engine_buffer_info(self.net._h, name.encode(), C.byref(p), None, None, None, None))
        return p

    def step(self, n, slot, pin=None):
        """pin: a pinned uint8 batch to send into input slot `slot` first (None: the slot's resident contents)"""
        from isegmi.dist import record_bytes
        ffi, net, L = self.ffi, self.net, self.ffi.lib()
        if pin is not None:
            net.upload_u8_async(pin, n, HI, WI, slot=slot)
        net.forward_device(n, slot)
        net.postprocess_device(HI, WI)
        nb = record_bytes(n, K, MD, self.proto_hw)
        rec = ffi.DeviceBuffer((nb,), np.uint8)
        got = C.c_int64()
        ffi.check(L.isegmi_yolact_pack_records(net._h, rec.ptr, C.c_int64(nb), 1, C.byref(got)))
        assert got.value == nb, (got.value, nb)
        pins = {"prior": ffi.PinnedBuffer((n, K), np.int32), "box_int": ffi.PinnedBuffer((n, K, 4), np.int64),
                "masks": ffi.PinnedBuffer((n, K, HI, WI), np.uint8)}
        for key, name in (("prior", "det.prior"), ("box_int", "det.box_int"), ("masks", "det.masks")):
            ffi.check(L.isegmi_engine_download_async(net._h, len(self.steps) & 1, pins[key].ptr, self._ptr(name), C.c_int64(pins[key].nbytes)))
        net.mark_step()
        self.steps.append((n, rec, pins))

    def results(self):
        from isegmi.dist import unpack_records
        out = []
        for i, (n, rec, pins) in enumerate(self.steps):
            self.net.wait_mark(len(self.steps) - 1 - i)     # this step's completion mark, not a device synchronisation
            r = unpack_records(rec.numpy(), n, K, MD, self.proto_hw)
            r = {k: np.array(v) for k, v in r.items()}
            for k, p in pins.items():
                r[k] = np.array(p.array)
            out.append(r)
        self.net.sync()
        for _, rec, pins in self.steps:
            rec.free()
            for p in pins.values():
                p.free()
        self.steps = []
        return out


def same(got, want, what):
    for k in FIELDS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


@pytest.fixture(scope="module")
def rig(ffi):
    """One Yolact R50 fp32 engine (max_batch 2, seeded random weights), four distinct seeded uint8 batches in pinned memory, and -- computed once,
    with one lane -- every batch's isolated result at bs = 2 and at bs = 1."""
    from isegmi.weights import yolact_state_dict
    import dataclasses
    from isegmi.yolact import Yolact, YolactConfig
    # (confidence threshold 0: with random weights nothing passes the default 0.05, and empty results would compare nothing)
    net = Yolact(yolact_state_dict(1234), dataclasses.replace(YolactConfig(), nms_conf_thresh=0.0), max_batch=2, input_size=SIZE)
    rng = np.random.default_rng(20261017)
    batches = [rng.integers(0, 256, (2, HI, WI, 3), dtype=np.uint8) for _ in range(4)]
    pins = []
    for b in batches:
        p = ffi.PinnedBuffer(b.shape, np.uint8)
        p.array[...] = b
        pins.append(p)
    net.set_param("step_overlap", 0.0)
    iso = {(i, n): isolated(net, b[:n]) for i, b in enumerate(batches) for n in (2, 1)}
    for i in range(1, 4):
        assert not np.array_equal(iso[(i, 2)]["score"], iso[(0, 2)]["score"]), "the batches must differ in their results"
    Queue.proto_hw = iso[(0, 2)]["proto"].shape[1:3]
    yield ffi, net, batches, pins, iso
    for p in pins:
        p.free()
    net.close()


def overlap_on(ffi, net):
    """-> True with two lanes in force; False when the engine REPORTS the fallback to one lane (the runtime gave lane 1's main stream no queue of its
    own).  Anything else -- one lane without that report -- fails."""
    net.sync()
    net.set_param("step_overlap", 1.0)
    ll = lane_layout(ffi, net)
    if ll[0] == 2:
        assert ll[1] == 0
        return True
    assert ll[0] == 1 and ll[1] == 1, "step_overlap 1 runs on one lane without reporting the fallback: %s" % ll
    return False


def test_lane_equality(rig):
    """Four batches into alternating slots, queued with no host wait: two lanes == one lane == isolated runs, for det.*, proto and the mask planes.
    (Four steps: each lane runs twice, each input slot is reused once.)"""
    ffi, net, batches, pins, iso = rig
    runs = {}
    for ov in (0, 1):
        if ov:
            overlap_on(ffi, net)
        else:
            net.sync(); net.set_param("step_overlap", 0.0)
        before = lane_layout(ffi, net)[17]
        q = Queue(ffi, net)
        for i in range(4):
            q.step(2, i & 1, pins[i])
        runs[ov] = q.results()
        ll = lane_layout(ffi, net)
        assert ll[17] - before == (2 if ll[0] == 2 else 0), "lane 1 takes every second forward exactly when two lanes are in force"
    for i in range(4):
        same(runs[1][i], runs[0][i], "two lanes vs one, step %d" % i)
        same(runs[1][i], iso[(i, 2)], "two lanes vs isolated, step %d" % i)
    # isolated forward + sync runs WITH the parameter on (they alternate lanes too; the synchronous upload's front end runs on lane 0's stream)
    for i in range(4):
        same(isolated(net, batches[i]), iso[(i, 2)], "isolated with two lanes, batch %d" % i)


def test_resident_slot(rig):
    """Four queued steps that all read slot 0 (a resident batch: both lanes read one input slot, each must wait for its upload itself)."""
    ffi, net, batches, pins, iso = rig
    overlap_on(ffi, net)
    q = Queue(ffi, net)
    q.step(2, 0, pins[3])
    for _ in range(3):
        q.step(2, 0)
    for i, r in enumerate(q.results()):
        same(r, iso[(3, 2)], "resident step %d" % i)


def test_upload_hazard(rig):
    """Steps i and i + 1 queued, then at once a different batch into the slot step i read: step i is unchanged (the write waits for step i's read of
    its input, which ran on the OTHER lane than the last forward), and a third step reads the new batch."""
    ffi, net, batches, pins, iso = rig
    overlap_on(ffi, net)
    for first in (0, 1):            # step i on lane 0 / on lane 1
        if first:
            net.upload_u8(batches[3]); net.forward_device(2); net.sync()   # shifts the lane counter by one
        q = Queue(ffi, net)
        q.step(2, 0, pins[0])
        q.step(2, 1, pins[1])
        q.step(2, 0, pins[2])       # its upload into slot 0 is enqueued right behind step i + 1
        r = q.results()
        for i in range(3):
            same(r[i], iso[(i, 2)], "hazard, first lane %d, step %d" % (first, i))


def test_batch_sizes_alternate(rig):
    """bs = 1, 2, 1, 2 on one engine, queued: every step equals its isolated run at that batch size."""
    ffi, net, batches, pins, iso = rig
    overlap_on(ffi, net)
    for order in ((1, 2, 1, 2), (2, 1, 1, 2)):    # the second order: each lane's consecutive forwards differ in M
        q = Queue(ffi, net)
        for i, n in enumerate(order):
            q.step(n, i & 1, pins[i])
        for i, r in enumerate(q.results()):
            same(r, iso[(i, order[i])], "bs order %s, step %d" % (order, i))


def test_layout(rig):
    """On: lane 1's main stream sits on a hardware queue that carries neither lane 0's main stream nor the tail -- or the engine reports that it fell
    back to one lane.  Off: one lane, and the ten-role layout is what it is with the parameter on (dealing lane 1 moves none of the ten)."""
    ffi, net, batches, pins, iso = rig
    names = ["main", "side0", "side1", "side2", "tail", "heads", "hs0", "hs1", "hs2", "copy"]
    ten = (C.c_int32 * 10)()
    net.sync(); net.set_param("step_overlap", 0.0)
    off = lane_layout(ffi, net)
    ffi.check(ffi.lib().isegmi_engine_stream_layout(net._h, ten, 10))
    assert off[0] == 1 and off[2:12] == list(ten), (off, list(ten))
    two = overlap_on(ffi, net)
    on = lane_layout(ffi, net)
    ffi.check(ffi.lib().isegmi_engine_stream_layout(net._h, ten, 10))
    assert on[2:12] == off[2:12] == list(ten), (on, off, list(ten))
    cls = dict(zip(names, on[2:12]))
    print("lane layout:", cls, "lane 1 main/side0-2:", on[12:16], "lanes", on[0], "fallback", on[1])
    if two:
        assert on[12] >= 0 and on[12] not in (cls["main"], cls["tail"]), (cls, on[12:16])
        assert all(c >= 0 for c in on[13:16])
    else:
        assert on[1] == 1 and on[0] == 1


def test_forced_off(rig):
    """multi_stream 0 and the hipGraph mode (capture and replay) run on one lane whatever the parameter says, and give the same results."""
    ffi, net, batches, pins, iso = rig
    overlap_on(ffi, net)
    try:
        net.set_param("multi_stream", 0.0)
        assert lane_layout(ffi, net)[0] == 1
        before = lane_layout(ffi, net)[17]
        for i in (0, 1):
            same(isolated(net, batches[i]), iso[(i, 2)], "multi_stream 0, batch %d" % i)
        ll = lane_layout(ffi, net)
        assert ll[16] == 1 and ll[17] == before
        net.set_param("multi_stream", 1.0)
        net.set_param("graph", 1.0)
        assert lane_layout(ffi, net)[0] == 1
        for rep in range(3):        # eager warm-up, capture + replay, replay
            same(isolated(net, batches[2]), iso[(2, 2)], "graph mode, run %d" % rep)
        cap, rp, fail = C.c_int64(), C.c_int64(), C.c_int64()
        ffi.check(ffi.lib().isegmi_engine_graph_stats(net._h, C.byref(cap), C.byref(rp), C.byref(fail)))
        ll = lane_layout(ffi, net)
        assert cap.value >= 1 and fail.value == 0 and ll[16] == 1 and ll[17] == before, (cap.value, fail.value, ll)
    finally:
        net.set_param("graph", 0.0)
        net.set_param("multi_stream", 1.0)

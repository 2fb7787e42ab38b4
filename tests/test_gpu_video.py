"""-m gpu: video mode (the track kernels of csrc/visualize.hip, centermask2_amd/video.py) against the tests' NumPy restatement of the
association rule (tests/video_ref.py) and of the picture (tests/video_visualize_ref.py).  Everything is compared bit for bit after every
frame: the track ids, the whole table (boxes, classes, ids, ttl and, in mask mode, areas and packed words) and the counters.  The IoU
values themselves are never compared: both sides divide in IEEE float64, and a last-bit difference could only show as a different match.

Shapes (new instances per frame, max_tracks): (0,1) and (1,1) are the smallest tables, (1,1) drops every survivor; (3,8) is less than a
wave; (65,130) is more than a wave per row and more old rows than the 16 waves of the workgroup take in one trip, and overflows 130 rows;
(100,256) and (200,1024) are the detector's usual count and the largest table.  Masks: 5x7 is one word, 37x53 is 31 words with a partial
last one, 64x65 has rows that straddle words."""
import numpy as np
import pytest
import torch

from centermask2_amd import InstanceTracker, VideoVisualizer, Visualizer, ops
from centermask2_amd._lib import CmkError
from centermask2_amd.structures import Boxes, Instances
from . import video_ref as V
from . import video_visualize_ref as VR
from . import visualize_ref as R

pytestmark = pytest.mark.gpu

FRAMES = 12


def instances_on(dev, size, f):
    inst = Instances(size, pred_boxes=Boxes(torch.from_numpy(f["boxes"]).to(dev)), scores=torch.from_numpy(f["scores"]).to(dev),
                     pred_classes=torch.from_numpy(f["classes"]).to(dev))
    if f.get("masks") is not None:
        inst.pred_masks = torch.from_numpy(f["masks"]).to(dev)
    return inst


def bits(a):
    """float32 array -> its bit patterns (NaN boxes compare equal to themselves)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def compare(tracker, ref, got_ids, want_ids, where):
    assert got_ids.dtype == torch.int32 and got_ids.is_cuda and got_ids.cpu().numpy().tolist() == want_ids.tolist(), where
    t = tracker.table()
    counters = t["counters"].cpu().numpy().tolist()
    want = ref.arrays()
    k = len(ref.tracks)
    assert counters[:3] == [k, ref.next_id, ref.dropped], (where, counters)
    assert (tracker.n_tracks, tracker.next_id, tracker.dropped) == (k, ref.next_id, ref.dropped)
    assert np.array_equal(bits(t["boxes"][:k].cpu().numpy()), bits(want["boxes"])), where
    for key in ("classes", "ids", "ttl"):
        assert np.array_equal(t[key][:k].cpu().numpy(), want[key]), (where, key)
    if ref.match == "mask":
        assert np.array_equal(t["areas"][:k].cpu().numpy(), want["areas"]), where
        assert np.array_equal(t["words"][:k].cpu().numpy(), V.pack_words(want["masks"]) if k else np.zeros((0, t["words"].shape[1]), dtype=np.int64)), where


def run_sequence(dev, n, cap, match, size, seed, pool_factor=1.5):
    frames = V.sequence(n, frames=FRAMES, seed=seed, size=size, with_masks=match == "mask", pool_factor=pool_factor)
    tracker, ref = InstanceTracker(match=match, max_tracks=cap), V.RefTracker(match=match, max_tracks=cap)
    matched = 0
    for k, f in enumerate(frames):
        inst = instances_on(dev, size, f)
        before = ref.next_id
        want = ref.update(f["boxes"], f["classes"], f["masks"])
        got = tracker.update(inst)
        assert inst.track_ids is got
        compare(tracker, ref, got, want, (n, cap, match, size, "frame", k))
        matched += int((want < before).sum())
    return tracker, ref, matched, frames


@pytest.mark.parametrize("n,cap", [(0, 1), (1, 1), (3, 8), (65, 130), (100, 256), (200, 1024)])
def test_box_sequences_match_the_restatement(dev, n, cap):
    tracker, ref, matched, _ = run_sequence(dev, n, cap, "box", (480, 640), seed=1000 + n, pool_factor=3.0 if n in (1, 65) else 1.5)
    if n >= 3:
        assert matched > 0 and ref.next_id > n, "the sequence matches some instances and numbers some new ones"
    if (n, cap) in ((1, 1), (65, 130)):
        assert ref.dropped > 0, "this shape overflows its table"
    if n == 200:
        assert ref.dropped == 0 and len(ref.tracks) > 256


@pytest.mark.parametrize("n,cap", [(3, 8), (65, 130)])
@pytest.mark.parametrize("size", [(5, 7), (37, 53), (64, 65)])
def test_mask_sequences_match_the_restatement(dev, size, n, cap):
    tracker, ref, matched, _ = run_sequence(dev, n, cap, "mask", size, seed=2000 + n + size[0], pool_factor=3.0 if n == 65 else 1.5)
    assert matched > 0
    if n == 65:
        assert ref.dropped > 0


def test_mask_mode_empty_and_smallest_tables(dev):
    for n, cap in ((0, 1), (1, 1)):
        _, ref, _, _ = run_sequence(dev, n, cap, "mask", (37, 53), seed=7 + n, pool_factor=3.0)
        assert (ref.dropped > 0) == (n == 1)


def test_reset_frame_size_and_packed_inputs(dev):
    """reset() forgets the tracks (the stale rows of the table are never read as tracks) and lets the frame size change; without it a new
    size is refused in mask mode and accepted in box mode; packed (words, areas) may be handed in."""
    size = (37, 53)
    tracker, ref, _, frames = run_sequence(dev, 3, 8, "mask", size, seed=11)
    other = V.sequence(3, frames=2, seed=12, size=(5, 7), with_masks=True)
    with pytest.raises(CmkError, match="5x7.*37x53.*reset"):
        tracker.update(instances_on(dev, (5, 7), other[0]))
    compare(tracker, ref, tracker.update(instances_on(dev, size, frames[0])), ref.update(frames[0]["boxes"], frames[0]["classes"], frames[0]["masks"]),
            "after a refused frame the table is as it was")
    tracker.reset()
    assert (tracker.n_tracks, tracker.next_id, tracker.dropped) == (0, 0, 0)
    ref = V.RefTracker(match="mask", max_tracks=8)
    for f in other:
        inst = instances_on(dev, (5, 7), f)
        words, areas = ops.mask_pack_bits(inst.pred_masks)
        no_masks = Instances((5, 7), pred_boxes=inst.pred_boxes, scores=inst.scores, pred_classes=inst.pred_classes)
        compare(tracker, ref, tracker.update(no_masks, words, areas), ref.update(f["boxes"], f["classes"], f["masks"]), "packed inputs after reset")
    box = InstanceTracker(max_tracks=8)
    two = dict(boxes=np.array([[0, 0, 10, 10], [20, 20, 40, 40]], dtype=np.float32), scores=np.ones(2, dtype=np.float32), classes=np.zeros(2, dtype=np.int64))
    a = box.update(instances_on(dev, size, two))
    b = box.update(instances_on(dev, (5, 7), two))                    # the same boxes in a frame of another size
    assert a.cpu().tolist() == [0, 1] == b.cpu().tolist()
    many = V.sequence(9, frames=1, seed=3)[0]
    with pytest.raises(CmkError, match=r"9 instances \(boxes \(9, 4\)\) but max_tracks = 8"):
        box.update(instances_on(dev, (480, 640), many))


def prepare_inputs(dev, n, seed):
    f = V.sequence(n, frames=1, seed=seed, size=(60, 90))[0]
    vis = Visualizer(class_names=["a", "bc"])
    t = vis._device_tables(dev)
    boxes, scores, classes = (torch.from_numpy(f[k]).to(dev) for k in ("boxes", "scores", "classes"))
    order = torch.from_numpy(np.array(R.draw_order(f["boxes"]), dtype=np.int64)).to(dev)
    args = (boxes, scores, classes, order, t["names"], t["name_lens"], t["num_names"], t["palette"], 60, 90, 1)
    return args, order.cpu().numpy()


def pack3(c):
    return c[0] | (c[1] << 8) | (c[2] << 16)


@pytest.mark.parametrize("n", [1, 64, 100])
def test_vis_prepare_ids(dev, n):
    """arange(n) with n <= 64 is vis_prepare bit for bit; any other ids change the three colour fields alone, to palette[id mod 64] (the
    remainder non-negative) and the edge and text colours derived from it.  Records are in draw order, ids by original instance."""
    args, order = prepare_inputs(dev, n, seed=40 + n)
    plain = ops.vis_prepare(*args, False)
    by_class = ops.vis_prepare(*args, True)
    if n <= 64:
        same = ops.vis_prepare_ids(*args, False, torch.arange(n, dtype=torch.int32, device=dev))
        assert torch.equal(same, plain)
    rng = np.random.RandomState(n)
    for ids in (rng.permutation(n), rng.randint(64, 100000, n), rng.randint(-1000, 0, n), np.full(n, 2 ** 31 - 1), np.full(n, -2 ** 31)):
        ids = ids.astype(np.int32)
        got = ops.vis_prepare_ids(*args, False, torch.from_numpy(ids).to(dev))
        assert torch.equal(got, ops.vis_prepare_ids(*args, True, torch.from_numpy(ids).to(dev))), "color_by_class is not consulted"
        got, want = got.cpu().numpy(), plain.cpu().numpy().copy()
        for j in range(n):
            col, edge, text = R.colours(int(ids[order[j]]), "BGR")
            want[j, 7], want[j, 16], want[j, 17] = pack3(col), pack3(edge), pack3(text)
        assert np.array_equal(got, want)
        assert got.shape == by_class.shape


def swap_frames(h, w, match):
    """Three frames of the same two objects (and a third that appears in the last) on one image: the detector's order swaps in frame 1."""
    rng = np.random.RandomState(5)
    image = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    boxes = np.array([[4, 5, 30, 28], [26, 12, 60, 34], [40, 2, 55, 11]], dtype=np.float32)
    masks = np.zeros((3, h, w), dtype=bool)
    ys, xs = np.mgrid[0:h, 0:w]
    masks[0] = ((xs - 17) / 12.0) ** 2 + ((ys - 16) / 10.0) ** 2 <= 1
    masks[1] = (xs >= 28) & (xs < 58) & (ys >= 14) & (ys < 33) & ((xs + ys) % 5 != 0)
    masks[2] = (xs >= 41) & (xs < 54) & (ys >= 3) & (ys < 10)
    scores = np.array([0.9, 0.8, 0.7], dtype=np.float32)
    classes = np.array([0, 0, 1], dtype=np.int64)
    frames = []
    for pick in ([0, 1], [1, 0], [2, 1, 0]):
        frames.append(dict(image=image, boxes=boxes[pick], scores=scores[pick], classes=classes[pick], masks=masks[pick] if match == "mask" else None,
                           all_masks=masks[pick]))
    return frames


@pytest.mark.parametrize("match", ["box", "mask"])
def test_video_visualizer_keeps_colours_when_the_order_swaps(dev, match):
    h, w = 37, 70
    frames = swap_frames(h, w, match)
    kw = dict(line_width=1, font_scale=1, input_format="RGB")
    want, want_ids = VR.render_video(frames, match=match, **kw)
    assert [v.tolist() for v in want_ids] == [[0, 1], [1, 0], [2, 1, 0]]
    vis, plain = VideoVisualizer(match=match, **kw), Visualizer(**kw)
    got, unstable = [], []
    for f in frames:
        inst = instances_on(dev, (h, w), f)
        img = torch.from_numpy(f["image"]).to(dev)
        got.append(vis.draw(img, inst).cpu().numpy())
        unstable.append(plain.draw(img, inst).cpu().numpy())
        assert inst.track_ids.cpu().numpy().tolist() == want_ids[len(got) - 1].tolist()
    for k in range(3):
        assert np.array_equal(got[k], want[k]), "frame {}: {} pixels differ from the restatement".format(k, int((got[k] != want[k]).any(axis=2).sum()))
    assert np.array_equal(got[0], unstable[0]) and not np.array_equal(unstable[0], unstable[1]), "colour by output index changes with the order"
    # nothing moved and only the order changed (the draw order goes by box area): with stable colours frames 0 and 1 are one picture
    assert np.array_equal(got[0], got[1])
    # pixels that one object alone owns, off every label plate: (16,12) in object 0's mask, (30,51) in object 1's; its box frame in box mode
    m0, m1 = frames[0]["all_masks"]
    assert m0[16, 12] and not m1[16, 12] and m1[30, 51] and not m0[30, 51] and R.colours(0, "RGB")[0] != R.colours(1, "RGB")[0]
    for y, x in ((16, 12), (30, 51)) if match == "mask" else ((16, 4), (34, 50)):
        assert (got[0][y, x] != frames[0]["image"][y, x]).any(), "the pixel is drawn"
        assert all(np.array_equal(got[k][y, x], got[0][y, x]) for k in range(3)), (y, x)
        assert not np.array_equal(unstable[1][y, x], unstable[0][y, x]), "by output index the same pixel changes colour"
    assert vis.tracker.next_id == 3 and vis.tracker.n_tracks == 3
    # an empty frame ages the table through draw as well, and reset starts again
    empty = Instances((h, w), pred_boxes=Boxes(torch.zeros((0, 4), device=dev)), scores=torch.zeros(0, device=dev),
                      pred_classes=torch.zeros(0, dtype=torch.int64, device=dev))
    out = vis.draw(torch.from_numpy(frames[0]["image"]).to(dev), empty)
    assert np.array_equal(out.cpu().numpy(), frames[0]["image"]) and vis.tracker.table()["ttl"][:3].cpu().tolist() == [7, 7, 7]
    vis.reset()
    assert vis.tracker.n_tracks == 0 and vis.tracker.next_id == 0

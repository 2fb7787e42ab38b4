"""-m gpu: the kernels after the FCOS head, one at a time, against a plain reference of the same operation: ROIAlign with both
level rules (the oracle's torchvision restatement), SAG-Mask spatial attention, the class-selected mask predictor, the MaskIoU input
pooling, the mask-IoU score, the FPN-norm helpers and the mask paste (float64 torch or exact fp32 torch).  Base case: the production
shapes (8 images x 50 slots, S = 14, C = 256, 80 classes, a 272-channel MaskIoU buffer with the pooled mask in channel 256) with
counts 0, partial and full; plus the edges where these kernels could go wrong."""
import math

import pytest
import torch
import torch.nn.functional as F

from centermask2_amd import ops
from centermask2_amd.ops import View
from oracle import centermask_oracle as O

from .helpers import close, close_abs

pytestmark = pytest.mark.gpu

N_IMG, TOPK = 8, 50
COUNTS = [50, 0, 23, 50, 1, 37, 50, 12]           # full, empty and partial images
SMALL = (3, 6, [6, 0, 4])                          # (images, slots, counts) of the off-production shapes
NAN = float("nan")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _valid_slots(counts, topk):
    """(N*topk,) bool: slot s of image n is valid iff s < counts[n]."""
    return (torch.arange(topk)[None, :] < torch.tensor(counts)[:, None]).reshape(-1)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------
# ROIAlign + level assignment (cmk_roi_align_pool)
# ---------------------------------------------------------------------------------------------------------------
ROI_PAD = (512, 640)                               # the padded batch: p3 64x80, p4 32x40, p5 16x20
ROI_SIZES = [(512, 640), (96, 128), (320, 448), (48, 64), (512, 320), (200, 256), (128, 640), (24, 40)]
SCALES = (1 / 8, 1 / 16, 1 / 32)


def _roi_boxes(seed):
    """(N_IMG, TOPK, 4) boxes in each image's frame: log-uniform sizes from 1/40 to 2.5 times the image's side with centres up to 30 %
    outside it, and in the first slots a sub-pixel box, two boxes wholly outside the map, a zero-width box, a box many times the
    padded batch (adaptive grid 5x4 on p5) and a box a quarter of image 0 (grid 3x3 on p3 there)."""
    g = _gen(seed)
    boxes = torch.empty(N_IMG, TOPK, 4)
    for n, (h, w) in enumerate(ROI_SIZES):
        bw = math.sqrt(h * w) * torch.empty(TOPK).uniform_(math.log(1 / 40), math.log(2.5), generator=g).exp()
        bh = bw * torch.empty(TOPK).uniform_(-1.0, 1.0, generator=g).exp()
        cx = torch.empty(TOPK).uniform_(-0.3, 1.3, generator=g) * w
        cy = torch.empty(TOPK).uniform_(-0.3, 1.3, generator=g) * h
        boxes[n] = torch.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)
        boxes[n, 0] = torch.tensor([0.5 * w, 0.5 * h, 0.5 * w + 0.3, 0.5 * h + 0.6])
        boxes[n, 1] = torch.tensor([ROI_PAD[1] + 40.0, 20.0, ROI_PAD[1] + 180.0, 90.0])
        boxes[n, 2] = torch.tensor([-300.0, -200.0, -100.0, -40.0])
        boxes[n, 3] = torch.tensor([10.0, 10.0, 10.0, 40.0])
        boxes[n, 4] = torch.tensor([-400.0, -300.0, 1500.0, 1200.0])
        boxes[n, 5] = torch.tensor([100.0, 50.0, 380.0, 306.0])
    return boxes


def _raw_levels(b, areas, by_area):
    """The level rules before the clamp (pooler.py:80-152), to show the boxes reach past both ends."""
    box_area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    if by_area:
        return torch.floor(4 + torch.log2(torch.sqrt(box_area) / 224 + 2.220446049250313e-16))
    return torch.ceil(5 - torch.log2(areas / box_area + 2.220446049250313e-16))


ROI_CASES = [(256, sr, aligned, by_area) for sr in (0, 2) for aligned in (True, False) for by_area in (False, True)] + \
            [(100, 0, True, False), (512, 0, True, False), (512, 2, False, True)]


@pytest.mark.parametrize("c,sr,aligned,by_area", ROI_CASES)
def test_roi_align_levels_and_features_match_oracle(dev, c, sr, aligned, by_area):
    """8 images of different areas: levels exactly the oracle's fp32 rule (each image's own area), invalid slots level -1 and zero
    features, valid features within the roi_feat bar of O.roi_pooler, channels >= C of the wider output buffer untouched.  C = 100
    leaves lanes idle; C = 512 makes every lane loop twice."""
    g = _gen(1000 + c)
    feats = [torch.randn((N_IMG, c, ROI_PAD[0] // st, ROI_PAD[1] // st), generator=g) for st in (8, 16, 32)]
    boxes = _roi_boxes(7)
    valid = _valid_slots(COUNTS, TOPK)
    areas = torch.tensor([float(h * w) for h, w in ROI_SIZES])
    y_cs = c + 16
    y = torch.full((N_IMG * TOPK, 14, 14, y_cs), NAN, device=dev)
    levels = ops.roi_align_ratio([View(f.permute(0, 2, 3, 1).contiguous().to(dev)) for f in feats], SCALES, boxes.to(dev),
                                 torch.tensor(COUNTS, dtype=torch.int32, device=dev), areas.to(dev), 14, sr, y, 3, aligned=aligned,
                                 assign_by_area=by_area, canonical_box_size=224.0, canonical_level=4)
    torch.cuda.synchronize()
    got, levels = y.cpu(), levels.cpu().long()

    per_image = [boxes[n, :k] for n, k in enumerate(COUNTS)]
    want, want_lv = O.roi_pooler(feats, per_image, ROI_SIZES, SCALES, 14, sr, "area" if by_area else "ratio", aligned, 224, 4)
    vb = boxes.reshape(-1, 4)[valid]
    va = areas.repeat_interleave(torch.tensor(COUNTS))
    # the inputs reach what the test is for: all three levels, the clamp at both ends, adaptive grids well above 2x2 ...
    assert sorted(set(want_lv.tolist())) == [0, 1, 2]
    raw = _raw_levels(vb, va, by_area)
    assert (raw < 3).any() and (raw > 5).any()
    if sr == 0:
        sc = torch.tensor(SCALES)[want_lv]
        side = torch.maximum((vb[:, 2] - vb[:, 0]) * sc, (vb[:, 3] - vb[:, 1]) * sc)
        assert (torch.ceil(side / 14) >= 3).any()
    # ... and, for the ratio rule, image 0's area would put some boxes on another level
    if not by_area:
        assert (O.assign_boxes_to_levels_by_ratio(vb, torch.full_like(va, float(areas[0]))) != want_lv).any()

    assert torch.equal(levels[valid], want_lv), "levels differ from the oracle's fp32 rule"
    assert (levels[~valid] == -1).all()
    assert torch.equal(got[~valid][..., :c], torch.zeros_like(got[~valid][..., :c])), "invalid slots must be zero"
    assert torch.isnan(got[..., c:]).all(), "channels >= C of the output buffer must be untouched"
    close(got[valid][..., :c].permute(0, 3, 1, 2), want, 1e-5, "roi_align features")


# ---------------------------------------------------------------------------------------------------------------
# SAG-Mask spatial attention (sam.py:23-28)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [14, 7, 28])
@pytest.mark.parametrize("c", [256, 4, 516])
def test_spatial_attention_matches_float64(dev, s, c):
    """x * sigmoid(conv3x3([mean_C x, max_C x])) on valid rows; rows at or beyond counts[n] are left bit for bit.  S = 28 has more
    pixels than the block has threads, C = 516 more channel quads than a wave has lanes."""
    n, topk, counts = (N_IMG, TOPK, COUNTS) if (s, c) == (14, 256) else SMALL
    g = _gen(2000 + 10 * s + c)
    x = torch.randn((n * topk, s, s, c), generator=g) * 2.0
    w = torch.randn(18, generator=g) * 0.5                    # (1, 2, 3, 3): [mean | max][kh][kw]
    valid = _valid_slots(counts, topk)
    x[~valid, :, :, ::2] = NAN                                 # a row the kernel touched would come out all NaN
    xd = x.to(dev)
    ops.spatial_attention_(xd, w.to(dev), torch.tensor(counts, dtype=torch.int32, device=dev), topk)
    torch.cuda.synchronize()
    got = xd.cpu()
    assert torch.equal(_bits(got[~valid]), _bits(x[~valid])), "slots at or beyond counts[n] must not be written"
    xv = x[valid].double().permute(0, 3, 1, 2)
    pooled = torch.cat([xv.mean(1, keepdim=True), xv.amax(1, keepdim=True)], 1)
    ref = xv * torch.sigmoid(F.conv2d(pooled, w.double().view(1, 2, 3, 3), padding=1))
    close(got[valid].permute(0, 3, 1, 2), ref, 2e-6, "spatial attention")


# ---------------------------------------------------------------------------------------------------------------
# class-selected mask predictor + sigmoid (mask_head.py:174-216)
# ---------------------------------------------------------------------------------------------------------------
def _poison(*shapes, dev):
    """Fill and free float32 blocks of these shapes, so the caching allocator hands NaN-filled memory to the next torch.empty of the
    same sizes: an output the kernel skipped would show as NaN instead of a lucky zero."""
    bufs = [torch.full(sh, NAN, device=dev) for sh in shapes]
    torch.cuda.synchronize()
    del bufs


@pytest.mark.parametrize("c,classes,want_logits", [(256, "mixed", True), (256, "mixed", False), (256, "agnostic", True),
                                                   (260, "mixed", True), (260, "mixed", False)])
def test_mask_predict_matches_float64(dev, c, classes, want_logits):
    """dec (R,S,S,(dh,dw),C) . predictor[cls[r]] + bias[cls[r]], then sigmoid, on the (2S,2S) grid; classes 0 and 79 and an
    all-zero class vector (class-agnostic masks); C = 260 has a channel tail past 256.  Invalid slots are exactly 0."""
    n, topk, counts = (N_IMG, TOPK, COUNTS) if c == 256 else SMALL
    s, k, r = 14, 80, n * topk
    g = _gen(3000 + c)
    valid = _valid_slots(counts, topk)
    dec = torch.full((r, s, s, 4 * c), NAN)
    dec[valid] = torch.rand((int(valid.sum()), s, s, 4 * c), generator=g)        # relu(deconv) >= 0
    pw = torch.randn((k, c), generator=g) * (2.0 / c) ** 0.5
    pb = torch.randn(k, generator=g) * 0.5
    if classes == "agnostic":
        cls = torch.zeros(r, dtype=torch.int64)
    else:
        cls = torch.randint(0, k, (r,), generator=g)
        cls[0], cls[1] = 0, 79
    _poison((r, 1, 2 * s, 2 * s), (r, 2 * s, 2 * s), dev=dev)
    out = ops.mask_predict(dec.to(dev), pw.to(dev), pb.to(dev), cls.to(dev), torch.tensor(counts, dtype=torch.int32, device=dev), topk,
                           want_logits=want_logits)
    torch.cuda.synchronize()
    masks, logits = (out[0].cpu(), out[1].cpu()) if want_logits else (out.cpu(), None)
    assert masks.shape == (r, 1, 2 * s, 2 * s)
    rows = valid.nonzero().squeeze(1)
    ref = torch.empty((len(rows), 2 * s, 2 * s), dtype=torch.float64)
    for part in range(0, len(rows), 64):
        ch = rows[part:part + 64]
        d = dec[ch].double().reshape(len(ch), s, s, 2, 2, c)
        lg = torch.einsum("rhwijc,rc->rhiwj", d, pw.double()[cls[ch]]) + pb.double()[cls[ch]].view(-1, 1, 1, 1, 1)
        ref[part:part + len(ch)] = lg.reshape(len(ch), 2 * s, 2 * s)
    close_abs(masks[valid, 0], torch.sigmoid(ref), 2e-6, "mask_predict masks")
    assert (masks[~valid] == 0).all(), "invalid slots must be exactly 0"
    if want_logits:
        close(logits[valid], ref, 1e-5, "mask_predict logits")
        assert (logits[~valid] == 0).all(), "invalid slots must be exactly 0"


# ---------------------------------------------------------------------------------------------------------------
# 2x2 mask pooling into the MaskIoU input, score calibration (maskiou_head.py:50-60,107-112)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,s,y_cs,y_co", [(N_IMG * TOPK, 14, 272, 256), (37, 7, 272, 256), (30, 9, 40, 33)])
def test_mask_pool_concat_exact(dev, r, s, y_cs, y_co):
    """Channel y_co = max_pool2d(masks, 2) bit for bit; the pad channels after it exactly 0 on a NaN-filled buffer; channels < y_co
    untouched."""
    g = _gen(4000 + s)
    masks = torch.rand((r, 2 * s, 2 * s), generator=g)
    y0 = torch.randn((r, s, s, y_cs), generator=g)
    y0[..., y_co:] = NAN
    y = y0.to(dev)
    ops.mask_pool_concat_(masks.to(dev), y, y_co)
    torch.cuda.synchronize()
    got = y.cpu()
    assert torch.equal(got[..., y_co], F.max_pool2d(masks[:, None], 2)[:, 0])
    assert torch.equal(got[..., y_co + 1:], torch.zeros_like(got[..., y_co + 1:])), "pad channels must be zeroed"
    assert torch.equal(_bits(got[..., :y_co]), _bits(y0[..., :y_co])), "feature channels must be untouched"


@pytest.mark.parametrize("r", [N_IMG * TOPK, 513, 1])
def test_mask_iou_score_exact(dev, r):
    g = _gen(5000 + r)
    iou = torch.rand((r, 80), generator=g)
    scores = torch.rand(r, generator=g)
    cls = torch.randint(0, 80, (r,), generator=g)
    cls[0] = 79
    cls[-1] = 0 if r > 1 else 79
    got = ops.mask_iou_score(iou.to(dev), scores.to(dev), cls.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), scores * iou[torch.arange(r), cls])


# ---------------------------------------------------------------------------------------------------------------
# FPN-norm helpers: nearest-2x top-down sum, LastLevelMaxPool
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hc,wc,h,w,c", [(2, 13, 20, 26, 40, 256), (2, 13, 20, 25, 39, 256), (1, 7, 5, 13, 10, 64), (3, 1, 1, 1, 2, 4)])
def test_upsample2x_add_exact(dev, n, hc, wc, h, w, c):
    g = _gen(6000 + h * w)
    y = torch.randn((n, c, h, w), generator=g)
    coarse = torch.randn((n, c, hc, wc), generator=g)
    want = y + F.interpolate(coarse, scale_factor=2, mode="nearest")[..., :h, :w]
    yv = ops.as_view(y.to(dev))
    ops.upsample2x_add_(yv, ops.as_view(coarse.to(dev)))
    torch.cuda.synchronize()
    assert torch.equal(yv.nchw().cpu(), want)


@pytest.mark.parametrize("n,h,w,c,cs,co", [(2, 25, 40, 256, 256, 0), (2, 13, 11, 64, 96, 16), (1, 7, 9, 100, 132, 28), (1, 1, 1, 4, 8, 4)])
def test_maxpool1x1s2_exact(dev, n, h, w, c, cs, co):
    """Every second pixel of a channel slice [co, co+C) of a wider buffer, odd sizes included."""
    t = torch.randn((n, h, w, cs), generator=_gen(7000 + h * w))
    got = ops.maxpool1x1s2(View(t.to(dev), co, c))
    torch.cuda.synchronize()
    assert torch.equal(got.nchw().cpu(), t[..., co:co + c].permute(0, 3, 1, 2)[:, :, ::2, ::2])


# ---------------------------------------------------------------------------------------------------------------
# mask paste (d2 _do_paste_mask)
# ---------------------------------------------------------------------------------------------------------------
def _paste_values(masks, boxes, img_h, img_w):
    """d2 _do_paste_mask before the threshold: the fp32 grid exactly as O.paste_masks builds it, grid_sample on float64 masks."""
    n = masks.shape[0]
    x0, y0, x1, y1 = torch.split(boxes, 1, dim=1)
    img_y = torch.arange(0, img_h, dtype=torch.float32) + 0.5
    img_x = torch.arange(0, img_w, dtype=torch.float32) + 0.5
    img_y = (img_y - y0) / (y1 - y0) * 2 - 1
    img_x = (img_x - x0) / (x1 - x0) * 2 - 1
    gx = img_x[:, None, :].expand(n, img_y.size(1), img_x.size(1))
    gy = img_y[:, :, None].expand(n, img_y.size(1), img_x.size(1))
    grid = torch.stack([gx, gy], dim=3)
    return F.grid_sample(masks[:, None].double(), grid.double(), align_corners=False)[:, 0]


@pytest.mark.parametrize("s", [28, 13])
def test_paste_masks_matches_grid_sample(dev, s):
    """300 x 530 image (three 256-wide x blocks, the last ragged): boxes inside, partly outside, larger than the image, under one
    pixel wide; every pixel whose float64 value is more than 1e-5 from the threshold is exact."""
    h, w = 300, 530
    g = _gen(8000 + s)
    fixed = torch.tensor([[50.0, 40.0, 250.0, 200.0], [-60.0, -30.0, 120.0, 90.0], [400.0, 220.0, 700.0, 420.0],
                          [-100.0, -80.0, 650.0, 400.0], [200.3, 50.0, 200.7, 250.0], [10.2, 10.1, 10.9, 10.6]])
    xy = torch.rand((6, 2), generator=g) * torch.tensor([w, h])
    wh = torch.rand((6, 2), generator=g) * 300 + 2
    boxes = torch.cat([fixed, torch.cat([xy - wh / 2, xy + wh / 2], 1)])
    masks = torch.rand((boxes.shape[0], s, s), generator=g)
    got = ops.paste_masks(masks.to(dev), boxes.to(dev), h, w)
    torch.cuda.synchronize()
    assert got.dtype == torch.bool and got.shape == (boxes.shape[0], h, w)
    v = _paste_values(masks, boxes, h, w)
    clear = (v - 0.5).abs() > 1e-5
    assert clear.double().mean() > 0.99
    assert torch.equal(got.cpu()[clear], (v >= 0.5)[clear])
    empty = ops.paste_masks(torch.zeros((0, s, s), device=dev), torch.zeros((0, 4), device=dev), h, w)
    assert empty.dtype == torch.bool and tuple(empty.shape) == (0, h, w)

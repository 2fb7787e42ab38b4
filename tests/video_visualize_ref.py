"""The picture restatement (tests/visualize_ref.py) with a colour index per instance: `render(..., color_index=ids)` is visualize_ref.render
with the colour of instance i taken from palette[ids[i] mod 64] instead of palette[i mod 64]; everything else about the picture is
visualize_ref's own code, which stays as it is.  `render_video` draws a sequence with the ids of tests/video_ref.py's RefTracker."""
import numpy as np

from . import video_ref as V
from . import visualize_ref as R


def render(image, boxes, scores, classes, color_index=None, **kw):
    """color_index: (n,) ints by original instance, or None for visualize_ref.render as it is.  visualize_ref.render looks its colours up
    through the module's `colours(k, input_format)` with k the instance index (color_by="instance"): the index is translated there."""
    if color_index is None:
        return R.render(image, boxes, scores, classes, **kw)
    assert kw.get("color_by", "instance") == "instance", "a colour index replaces the instance index"
    ids = [int(v) for v in color_index]
    assert len(ids) == len(np.asarray(boxes).reshape(-1, 4))
    plain = R.colours
    R.colours = lambda k, input_format: plain(ids[k], input_format)
    try:
        return R.render(image, boxes, scores, classes, **kw)
    finally:
        R.colours = plain


def render_video(frames, match="box", tracker_kw=None, **kw):
    """frames: dicts of image, boxes, scores, classes and masks (or None).  -> (pictures, ids per frame) with one RefTracker over all."""
    tr = V.RefTracker(match=match, **(tracker_kw or {}))
    pictures, all_ids = [], []
    for f in frames:
        ids = tr.update(f["boxes"], f["classes"], f.get("masks"))
        all_ids.append(ids)
        pictures.append(render(f["image"], f["boxes"], f["scores"], f["classes"], color_index=ids, masks=f.get("masks"), **kw))
    return pictures, all_ids

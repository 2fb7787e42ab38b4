"""-m gpu: evaluation.CityscapesInstanceEvaluator on GPU Instances (the table from ops.mask_label_counts, csrc/eval/label_counts.hip)
against the same Instances on the host (cityscapes_eval.label_counts_host): identical records and identical results on the two-image,
three-class case of tests/cityscapes_ref.py, which the CPU tests hold to the brute-force restatement."""
import math

import pytest

from centermask2_amd.evaluation import CityscapesInstanceEvaluator
from tests import cityscapes_ref as R

pytestmark = pytest.mark.gpu


def test_gpu_instances_and_their_cpu_copies_score_alike(dev, monkeypatch):
    from centermask2_amd import cityscapes_eval as ce, ops
    gt, preds = R.two_image_case()
    inputs = [{"file_name": "leftImg8bit/val/aachen/{}_leftImg8bit.png".format(n)} for n in R.NAMES]
    on_gpu = [{"instances": R.instances_of(preds[n], device=dev)} for n in R.NAMES]
    on_cpu = [{"instances": o["instances"].to("cpu")} for o in on_gpu]
    calls = {"device": 0, "host": 0}
    device_path, host_path = ops.mask_label_counts, ce.label_counts_host
    monkeypatch.setattr(ops, "mask_label_counts", lambda *a: calls.__setitem__("device", calls["device"] + 1) or device_path(*a))
    monkeypatch.setattr(ce, "label_counts_host", lambda *a: calls.__setitem__("host", calls["host"] + 1) or host_path(*a))
    a, b = CityscapesInstanceEvaluator(ground_truth=gt), CityscapesInstanceEvaluator(ground_truth=gt)
    a.process(inputs, on_gpu)
    assert calls == {"device": 2, "host": 0}                            # selected by where the input lies
    b.process(inputs, on_cpu)
    assert calls == {"device": 2, "host": 2}
    assert a._predictions == b._predictions and sum(len(p["preds"]) for p in a._predictions) == 17
    ra, rb = a.evaluate()["segm"], b.evaluate()["segm"]
    assert set(ra) == set(rb) and 0 < ra["AP"] < 100
    for k in ra:
        assert ra[k] == rb[k] or (math.isnan(ra[k]) and math.isnan(rb[k])), k
    want = R.evaluate(R.bitmap_images(gt, preds))
    assert abs(ra["AP"] - 100 * want["AP"]) <= 1e-10 and abs(ra["AP50"] - 100 * want["AP50"]) <= 1e-10

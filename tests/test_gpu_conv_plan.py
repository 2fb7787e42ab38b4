"""-m gpu: the profiled launch path of ops.py (ops.PROFILE a list) records each conv under the kernel name and the executed FLOPs that the
library's plan of the launch gives (cmk_conv_plan), and launches what the unprofiled path launches.  The literals are the answers of the
Python mirrors this replaced (the three profile rows of tests/golden/conv_plan_cases.json; DESIGN.md, "The plan golden")."""
import pytest
import torch

from centermask2_amd import ops
from centermask2_amd.ops import View

pytestmark = pytest.mark.gpu

# (k, stride, H, W, Cin, Cout, forced variant, pool, kernel, executed FLOPs)
CASES = [(1, 1, 16, 16, 32, 256, (8, 32, 2), True, "conv_pw_kernel<2, true, false, false, false, 0>", 4194304),
         (3, 1, 12, 40, 32, 32, (6, 16, 1), False, "conv_wino6_kernel<false, 0>", 2359296),
         (3, 2, 16, 16, 32, 64, None, False, "conv_igemm_kernel<1, 1, 1, 1, 32, true>", 4718592)]


@pytest.mark.parametrize("k,stride,h,w,cin,cout,tv,pool,kernel,executed", CASES)
def test_profiled_launch_names_the_kernel_and_runs_the_same_conv(monkeypatch, k, stride, h, w, cin, cout, tv, pool, kernel, executed):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(7)
    pc = ops.PackedConv(torch.randn(cout, cin, k, k, generator=g) * 0.1, torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1, dev,
                        stride=stride)
    x = View(torch.randn(1, h, w, cin, generator=g).to(dev))
    monkeypatch.setattr(ops, "FORCE_VARIANT", tv)
    monkeypatch.setattr(ops, "AUTOTUNE", False)          # tv None: the library's untuned choice
    outs, pools = [], []
    for profile in ([], None):
        monkeypatch.setattr(ops, "PROFILE", profile)
        pooled = [] if pool else None
        outs.append(ops.conv_out(x, pc, relu=True, pool=pooled).t)
        torch.cuda.synchronize()
        if pool:
            assert len(pooled) == 1
            pools.append(pooled[0][0])
        if profile is not None:
            assert len(profile) == 1 and len(profile[0]) == 7
            name, flops, nbytes, e0, e1, shape, exe = profile[0]
            assert name == kernel and exe == executed
            assert flops == 2.0 * outs[0].shape[1] * outs[0].shape[2] * cin * cout * k * k and shape == (1, h, w, cin, cout, k, stride)
            assert e0.elapsed_time(e1) > 0.0
    assert torch.equal(outs[0], outs[1])
    assert not pool or torch.equal(pools[0], pools[1])

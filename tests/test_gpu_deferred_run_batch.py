"""The one ``run_batch`` of ctdet, multi_pose and ddd (BaseDetector): the probe's events around the same rows, on
the deferred-heads plan, and the deferral following options that change after construction.
resdcn_18 at the smallest inputs the plan tests of the three tasks use; B = 1 and K = 40: three 16-cell groups per
image, the last one partial."""
import contextlib
import functools
import sys

import pytest
import torch

from centernet_amd import native, synth

pytestmark = pytest.mark.gpu

TASKS = {
    "ctdet": (["--input_res", "128"], (128, 128), ("wh", "reg")),
    "multi_pose": (["--input_res", "128"], (128, 128), ("wh", "hps", "reg")),
    "ddd": (["--input_h", "128", "--input_w", "384"], (128, 384), ("dep", "rot", "dim", "wh", "reg")),
}
# an option changed after construction with which the task defers nothing
DENSE = {"ctdet": ("flip_test", True), "multi_pose": ("flip_test", True), "ddd": ("K", 130)}


@functools.lru_cache(maxsize=None)
def _detector(task):
    from centernet_amd.detectors import detector_factory
    from centernet_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        opt = opts().init([task, "--arch", "resdcn_18", "--K", "40"] + TASKS[task][0])
        det = detector_factory[opt.task](opt)
    synth.fill_state_dict_(det.model, 317)
    det.model.invalidate_plans()
    return det


def _cached_plans(m):
    return list(m.__dict__["_plans"].values())


@pytest.mark.parametrize("task", list(TASKS))
def test_run_batch_probe_same_rows_on_the_deferred_plan(dev, task):
    det, m = _detector(task), _detector(task).model
    (h, w), names = TASKS[task][1:]
    x = synth.images(1, h, w, seed=5).to(dev)
    want = det.run_batch(x).clone()
    m.drop_plans()
    probe = {"event_after": {0}}
    got = det.run_batch(x, probe=probe).clone()
    ran = _cached_plans(m)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    # the start of the launch list and the boundary behind launch 0; before and after the decode
    assert len(probe["net_events"]) == 2 and len(probe["dec_events"]) == 2
    assert probe["net_events"][0].elapsed_time(probe["net_events"][1]) > 0
    assert probe["dec_events"][0].elapsed_time(probe["dec_events"][1]) > 0
    assert probe["net_events"][1].elapsed_time(probe["dec_events"][0]) > 0      # the network, then the decode
    # one plan was built and run: the deferred one, which is what plan_for answers
    plan = m.plan_for(1, h, w, x.device)
    assert len(ran) == 1 and ran[0] is plan
    assert m.deferral() == names and plan.deferred is not None and plan.deferred.names == names


@pytest.mark.parametrize("task", list(TASKS))
def test_run_batch_follows_options_changed_after_construction(dev, task):
    det, m = _detector(task), _detector(task).model
    (h, w), names = TASKS[task][1:]
    x = synth.images(1, h, w, seed=6).to(dev)
    det.run_batch(x)
    assert m.deferral() == names
    key, value = DENSE[task]
    before = getattr(det.opt, key)
    setattr(det.opt, key, value)
    try:
        m.drop_plans()
        try:
            got = det.run_batch(x).clone()
        except native.NativeError as e:
            # ddd: as the library stands no image-level decode takes more than 128 rows, so the dense decode of
            # the K = 130 maps refuses (tests/test_gpu_ddd_heads_at_cells.py::test_nothing_deferred_above_128_rows);
            # the network has run by then, which is what this test is about
            assert task == "ddd" and "cn_ddd_decode_f32" in str(e)
            got = None
        ran = _cached_plans(m)
        assert m.deferral() == () and m.deferred_names() == ()
        plan = m.plan_for(1, h, w, x.device)
        assert len(ran) == 1 and ran[0] is plan and plan.deferred is None
        assert all(n in plan.outputs for n in names)
        with torch.no_grad():
            maps = m(x, borrow=True)[-1]                           # the dense plan's maps, the dense decode
            if got is None:
                with pytest.raises(native.NativeError, match="cn_ddd_decode_f32"):
                    det._decode_batch(maps)
            else:
                dense = det._decode_batch(maps)
                torch.cuda.synchronize()
                assert got.shape[:2] == (1, det.opt.K) and torch.equal(got, dense)
    finally:
        setattr(det.opt, key, before)
    det.run_batch(x)
    assert m.deferral() == names and m.plan_for(1, h, w, x.device).deferred is not None

"""box-delivery-v0 / area-clearing-v0: enable_timing / kernel_time_ms count one event triple per library call that steps or drains, and none for a reset."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

STEP_LIMIT = 500   # the path loop's limit, lowered through bd_overrides as the other small tests do


def _env(task):
    if task == "bd":
        from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
        return BatchedBoxDeliveryEnv(4, num_trials=2, seed=7, bd_overrides={"step_limit": STEP_LIMIT})
    from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv
    return BatchedAreaClearingEnv(4, cfg={"env": "clear_env", "agent": {"action_type": "heading"}}, num_trials=4, bd_overrides={"step_limit": STEP_LIMIT})


@pytest.mark.parametrize("task", ["bd", "ac"])
def test_timing_counts_steps_slices_and_drains_not_resets(task):
    env = _env(task)
    E, dev = env.num_envs, env.device
    g = torch.Generator().manual_seed(11)
    act = lambda: (torch.rand(E, generator=g, dtype=torch.float64) * 2 - 1).to(dev)   # noqa: E731
    env.enable_timing(True)
    env.reset()
    mask = torch.zeros(E, dtype=torch.uint8, device=dev)
    mask[1] = 1
    env.reset(mask)
    # 1. three lock-step steps: three triples; the resets above took none
    for _ in range(3):
        env.step(act())
    physics_ms, raster_ms, n = env.kernel_time_ms()
    print(task, "step x3:", physics_ms, raster_ms, n)
    assert n == 3
    assert physics_ms > 0
    assert math.isfinite(raster_ms) and raster_ms >= 0
    assert env.kernel_time_ms()[2] == 0   # reading the timers starts the count over
    # 2. two slices and the drain that closes them
    env.step_async(act(), budget=120)
    env.step_async(act(), budget=120)
    assert env.async_open
    env.drain()
    n = env.kernel_time_ms()[2]
    print(task, "step_async x2 + drain:", n)
    assert n == 3
    # 3. a queue round: the recv's slice call and the close's drain are counted, the reset of the send is not (nor is the open, which steps nothing)
    q = env.async_queue(2, budget=120)
    ids = q.recv()[0]
    reset = torch.tensor([1, 0], dtype=torch.uint8, device=dev)
    q.send(torch.zeros(2, dtype=torch.float64, device=dev), ids, reset)
    q.close()
    n = env.kernel_time_ms()[2]
    print(task, "queue recv + send(reset) + close:", n)
    assert n == 2
    env.close()

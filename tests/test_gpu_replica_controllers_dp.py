"""config.ada_target, config.lecam_weight and config.skip_nonfinite_updates with replicas on the HIP backend
(tools/dp_controllers_one_gpu.py under torch.distributed.run): two ranks share the one GPU over gloo (RCCL
refuses two ranks per device) and end every step with bit-identical parameters and controllers, a NaN on one rank skipping the
step on both; and one rank on RCCL with the controllers' all-gathers inside the captured graph, bit-equal to the single-process
step.  At most three processes are alive: this one's child (torchrun) and its two ranks.  The worker asserts; this file checks
its exit status and its last line."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _torchrun(nproc, timeout, **env):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "dp_controllers_one_gpu.py")]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout


def test_two_gloo_ranks_on_one_gpu_hold_the_same_controllers_and_skip_together():
    """float32, eager, per-device batch 2, all three switches on, GradSync(schedule="exclusive"): three steps with parameters,
    ada.state, lecam.state and guard.counters bit-identical across the ranks, p > 0, anchors non-zero; then rank 1's z carries
    a NaN in step 2 -- both ranks keep step 1's parameters, both count two skipped half steps, step 3 proceeds."""
    out = _torchrun(2, 300, DPC_MODE="step")
    print(out[-800:])
    assert "controllers step OK" in out


def test_rccl_inside_the_graph_one_rank_is_the_single_process_step():
    """backend nccl, world 1, bfloat16, all three switches on: one eager step + three replays with the exclusive exchange (the
    controllers' all-gathers captured into the hipGraph; one row each) are bit-equal to four eager steps with grad_sync=None --
    parameters, moments, EMA, ada.state, lecam.state, guard.counters, the verdict and the metrics."""
    out = _torchrun(1, 300, DPC_MODE="graph")
    print(out[-2000:])
    assert "controllers graph OK" in out

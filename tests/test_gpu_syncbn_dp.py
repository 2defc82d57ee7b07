"""Cross-replica BatchNorm groups on the HIP backend (tools/dp_syncbn_one_gpu.py under torch.distributed.run): two ranks share
the one GPU over gloo (RCCL refuses two ranks per device) -- the generator's forward and backward against the float64 oracle
on the CONCATENATED batch, one whole train_step with the ranks ending identical -- and one rank on RCCL with the group's
collectives inside the captured graph.  At most three processes are alive: this one's child (torchrun) and its two ranks."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# norm-relative per leaf: the gate of tests/test_gpu_dp.py::test_two_ranks_hip_backend_match_averaged_oracle.  For the GRADIENT leaves
# the denominator is floored at 1e-2 x the network's RMS gradient x sqrt(numel) (tests/syncbn_reference.errors, the floor of
# tests/test_host_logic.py::test_gradients_match): leaves with a small true gradient are gated against that floor, not their norm.
GATE = 1e-3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _torchrun(nproc, timeout, **env):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "dp_syncbn_one_gpu.py")]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout


def test_generator_with_one_group_of_two_ranks_matches_the_oracle_on_the_concatenated_batch(tmp_path):
    """float32, get_test_config(), per-device batch 2, batch_norm_group_size = 4.  Images per rank against their slice, all 22
    batch_stats leaves (bit-equal between the ranks), the SUM of the ranks' parameter gradients: each within 1e-3
    norm-relative per leaf (gradient leaves: with the floored denominator, see GATE) of oracle.torch_ref.generator in float64 on the batch of 4.  Control: batch_norm_group_size = -1
    must miss by more than 10 x the gate on the images and on a batch_stats leaf (the CPU oracle alone: 0.29 and 0.72)."""
    from tests import syncbn_reference as S
    assert "syncbn generator OK" in _torchrun(2, 600, SYNCBN_MODE="generator", SYNCBN_DUMP=str(tmp_path))
    load = lambda group: [torch.load(os.path.join(tmp_path, f"generator_{group}_rank{r}.pt")) for r in range(2)]
    ranks = load(4)
    assert len(ranks[0]["bn"]) == 22
    for (p, a), (_, b) in zip(ranks[0]["bn"], ranks[1]["bn"]):
        assert torch.equal(a, b), f"running statistics differ between the ranks at {p}"
    e = S.errors(ranks)
    print("HIP, two gloo ranks on one GPU, one BatchNorm group vs float64 oracle on the concatenated batch:", e)
    c = S.errors(load(-1))
    print("control, batch_norm_group_size = -1:", c)
    assert e["img"] < GATE and e["bn"] < GATE and e["grad"] < GATE, e
    assert c["img"] > 10 * GATE and c["bn"] > 10 * GATE, c


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_train_step_with_groups_keeps_the_ranks_identical(dtype):
    """one train_step, GradSync(schedule="exclusive"), one group of both ranks: finite, G / D parameters and G's batch_stats
    torch.equal across the ranks; GradSync(schedule="overlapped") with groups raises ValueError (asserted in the worker)."""
    assert f"syncbn step OK {dtype}" in _torchrun(2, 600, SYNCBN_MODE="step", SYNCBN_DTYPE=dtype)


def test_rccl_inside_the_graph_one_rank():
    """backend nccl, world 1, batch_norm_group_size = the per-device batch: the group's all-gathers are captured into the
    hipGraph.  One eager step + three replays are bit-equal to four eager steps of the same configuration and to four eager
    steps with batch_norm_group_size = -1 (parameters, batch_stats, losses)."""
    out = _torchrun(1, 900, SYNCBN_MODE="graph", SYNCBN_DTYPE="bfloat16")
    print(out[-1500:])
    assert "syncbn graph OK bfloat16" in out

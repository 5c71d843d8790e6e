"""The order of calls must not matter to a kernel's dynamic LDS.  The launch ledger (csrc/launch_ledger.hpp) raises a kernel's
reservation to what each launch passes, so a process that meets a small shape first must still launch the large one, and the small
one again after it.  tests/_launch_order_child.py does exactly that, in a process of its own (in this one, earlier tests have
raised the marks already), for every family of DESIGN.md 3.6.3 and for one kernel that used to reserve a compile-time maximum
once; each call is held to the family's own GPU test against its reference."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("gru_seq_bwd_scalar_stream", "dec_step_generic", "latent_step", "code_step", "code_step_attention", "vq_assign_generic",
            "vq_assign_split", "vq_assign_packed_2_tiles", "vq_assign_packed_4_tiles", "vq_soft_fused", "vae_latent", "dec_chain",
            "silhouette_samples")


def test_small_then_large_then_small_in_a_fresh_process():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_launch_order_child.py")], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    done = [line[3:] for line in run.stdout.splitlines() if line.startswith("ok ")]
    assert done == [f"{name} {step}" for name in FAMILIES for step in ("small", "large", "small again")]

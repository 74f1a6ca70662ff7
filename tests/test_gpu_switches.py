"""Every development switch of libgg (GG_*; read only when GG_DEV_SWITCHES is set) selects a kernel or schedule that is ALSO a product path --
the fallback the default schedule takes for shapes its fast kernels do not cover (channel counts that are not multiples of 4, single
windows, K above the prologue table, leading dimensions that are not multiples of 32, ...).  This file runs the same training-step parity check the default path gets (tools/switch_parity.py:
TinyViT-5M step vs the CPU oracle, fp32 and bf16 modes, per-tensor gradients) with the switches set, in groups, one subprocess per group
(the library reads a switch once per process).  The depthwise 3x3 family has no kernel switch: it runs one kernel per route, and only its
BatchNorm fusions (GG_NO_FUSE_DW_S1 / _S2, GG_NO_FUSE_BNBWD / _EPI) can be taken off."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GROUPS = {
    # every fusion off, every multi-window / resident / ring form replaced by its plain fallback
    "plain_fallbacks": dict(GG_NO_FUSE_DW_S1="1", GG_NO_FUSE_DW_S2="1", GG_NO_FUSE_BNBWD="1", GG_NO_BNGEMM="1", GG_NO_PRO="1", GG_F32_NO_FUSE="1", GG_NO_LN_COLSUM="1",
                            GG_ATTN_SMALL="0", GG_ATTN_FLASH_NO_RES="1",
                            GG_GEMM_F32_ROWS_EPI="0", GG_ATTN_NO_DS_SCRATCH="1", GG_ATTN_NO_FUSED_BWD="1", GG_ATTN_FWD_NO_TAIL="1", GG_GEMM_F32_PRO_RING="0", GG_GEMM_F32_NO_W96="1",
                            GG_ATTN_NO_SPLIT="1", GG_GEMM_DMA="0", GG_GEMM_TILE="n", GG_GEMM_F32_NO_SMALL="1", GG_SWITCH_PARITY_FROZEN="1"),
    # the older kernel generation: the depthwise data gradient without its act'(BN) epilogue, the fp32 GEMM's general epilogue with 64-byte-run stores, the
    # register-staged prologue GEMMs (the form K > 384 takes; GG_GEMM_F32_NO_PERSIST gives them one workgroup per tile -- at this test's shapes the
    # grid is below their resident count either way, so it is exercised, not distinguished)
    "older_kernels": dict(GG_NO_FUSE_BNBWD_EPI="1", GG_GEMM_F32_ROWS_EPI="0", GG_GEMM_F32_PRO_RING="0", GG_GEMM_F32_NO_PERSIST="1",
                          GG_GEMM_F32_NO_PAIR_STORE="1", GG_GEMM_TILE="w",
                          GG_ATTN_NO_FUSED_BWD="1", GG_ATTN_NO_SPLIT="1", GG_GEMM_F32_NO_SPLITK="1", GG_GEMM_F32_SMALL_MAX="64", GG_SWITCH_PARITY_FROZEN="1"),       # (the streaming two-pass attention backward with the dS hand-off: the form windows beyond 256 tokens take)
    # the single-pass attention backward with one wave per key strip (no cooperative tail strip): the form every window whose strip count is not 4 n + 1 takes
    "attention_no_tail": dict(GG_ATTN_FUSED_NO_TAIL="1", GG_ATTN_NO_SPLIT="1", GG_SWITCH_PARITY_FROZEN="1"),
    # the f32-MFMA window attention (the form head dim 64 and windows other than 7 x 7 / 12 x 12 / 14 x 14 take) with everything else at its default; the
    # 16-bit LDS-DMA GEMM in its 256 x 256 geometry wherever the shape allows it
    "attention_f32_mfma_gemm16_256": dict(GG_ATTN_NO_SPLIT="1", GG_GEMM_DMA_TILE="256"),
    # the default schedule with every parameter trainable (unfused BatchNorm / weight-gradient paths of all stages) and under the freeze policy
    "default_unfrozen": dict(),
    "default_frozen": dict(GG_SWITCH_PARITY_FROZEN="1"),
}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_parity_under_switch_group(group):
    env = dict(os.environ, GG_DEV_SWITCHES="1", **GROUPS[group])
    env.pop("GG_PRECISION", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "switch_parity.py")], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count("-> ok") == 2


def test_switches_are_inert_without_the_dev_gate(tmp_path):
    """Without GG_DEV_SWITCHES a GG_* switch must not change anything: with switches set that would change the launch schedule if the gate leaked
    (the prologue and depthwise fusions off), the step is correct and issues exactly the launches (category, flop, bytes per launch) of a run
    without any GG_* switch."""
    base = {k: v for k, v in os.environ.items() if not k.startswith("GG_") or k == "GG_LIB"}
    logs = {}
    for name, switches in (("none", {}), ("ungated", dict(GG_NO_PRO="1", GG_NO_FUSE_DW_S1="1", GG_F32_NO_FUSE="1"))):
        log = tmp_path / f"{name}.json"
        env = dict(base, GG_SWITCH_PARITY_FROZEN="1", GG_SWITCH_PARITY_LAUNCH_LOG=str(log), **switches)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "switch_parity.py")], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0 and r.stdout.count("-> ok") == 2, (name, r.stdout[-2000:], r.stderr[-2000:])
        logs[name] = json.loads(log.read_text())
    assert len(logs["none"]) > 0
    assert logs["ungated"] == logs["none"]

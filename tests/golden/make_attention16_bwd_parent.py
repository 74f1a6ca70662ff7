"""Writes tests/golden/attention16_bwd_parent.npz: the bits (int16 view) of dqkv of gg_attention_flash16_bwd (head dim 64, include/gg_attn16b.h) on the N = 17, 65,
129 ``plain`` and ``late`` cases of tests/attention16_bwd_cases.py, with out / lse from gg_attention_flash16_fwd.  Run it on the GPU with a libgg.so built from the
commit BEFORE csrc/attention_flash16_bwd.hip gained the head-dim-32 window kernels; tests/test_gpu_attention16_win_bwd.py holds every later build to those bits.
    python tests/golden/make_attention16_bwd_parent.py [out.npz]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from geoguessr_ai_amd import ops          # noqa: E402
from tests import attention16_bwd_cases as B          # noqa: E402

CASES = [(N, cls) for N in (17, 65, 129) for cls in ("plain", "late")]


def parent_bits():
    store = {}
    for N, cls in CASES:
        c = B.get_case(N, cls)
        kw, qkv, dout = B.kw_of(c), c["qkv"].cuda(), c["dout"].cuda()
        out, lse = ops.attention_flash16(qkv, **kw, want_lse=True)
        dqkv = ops.attention_flash16_bwd(qkv, out, lse, dout, **kw)
        store[f"dqkv_{N}_{cls}"] = dqkv.contiguous().view(torch.int16).cpu().numpy()
    return store


if __name__ == "__main__":
    store = parent_bits()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "attention16_bwd_parent.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **store)
    print("wrote", path, {k: v.shape for k, v in store.items()})

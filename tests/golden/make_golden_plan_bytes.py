"""Writes tests/golden/tinyvit_plan_bytes_parent.json: gg_tinyvit_workspace_bytes_masked of the five variants at their native size, batch 8, training, in every
arithmetic mode, for the masks None and freeze_all_but_last_stage, with activation recompute off and on.  Run ONCE with the build of the commit in front of the
padded-window change (tests/test_window_pad_cpu.py holds later builds to these totals: a size that divides keeps its plan to the byte).  Host code: no GPU."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def plan_bytes():
    from geoguessr_ai_amd import _lib as L
    from geoguessr_ai_amd.models.tinyvit import VARIANTS, make_cfg, _tensor_table
    out = {}
    for name in VARIANTS:
        for precision in ("bf16", "fp32", "fp32_split"):
            for rc in (0, 1):
                cfg, _, _ = make_cfg(name, precision=precision, grad_checkpointing=bool(rc))
                table = _tensor_table(cfg)
                freeze = bytes(int(t["kind"] == 0 and not t["name"].startswith(("stages.0.", "stages.1.", "stages.2."))) for t in table)
                for label, mask in (("none", None), ("freeze", freeze)):
                    n = L.lib().gg_tinyvit_workspace_bytes_masked(C.byref(cfg), 8, 1, mask)
                    assert n > 0, L.lib().gg_last_error().decode()
                    out[f"{name}/{precision}/{label}/rc{rc}"] = n
    return out


if __name__ == "__main__":
    path = os.path.join(ROOT, "tests", "golden", "tinyvit_plan_bytes_parent.json")
    values = plan_bytes()
    with open(path, "w") as f:
        json.dump(values, f, indent=1, sort_keys=True)
    print("wrote", path)

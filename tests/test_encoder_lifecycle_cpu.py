"""``EncoderRuntime`` (models/flat.py), the step lifecycle under ``TinyVitBackbone`` and CLIP's ``_VisionModel``, on the CPU and without libgg.so:
stubs inherit each model's refusal texts (and CLIP's toggle override) but take their byte counts from a dict, record the hook calls and keep a
six-tensor CPU parameter table.  The expected texts are literals of what the two mirrors raised before they shared this class."""
import weakref
from types import SimpleNamespace

import pytest
import torch

from geoguessr_ai_amd._lib import GgError
from geoguessr_ai_amd.models.flat import EncoderNode, EncoderRuntime
from geoguessr_ai_amd.models.tinyvit import TinyVitBackbone
from geoguessr_ai_amd.pretrain.clip_embedder import _VisionModel

NAMES = ["stem.weight", "stem.bias", "blocks.0.weight", "blocks.0.bias", "blocks.1.weight", "head.weight"]


class _Hooks:
    def __init__(self):
        EncoderRuntime.__init__(self)          # (not the model's: that one asks the library for its tensor table)
        self.cfg = SimpleNamespace(recompute=0)
        self.table = [dict(name=n, offset=8 * i, numel=5, shape=(5,), kind=0, index=i) for i, n in enumerate(NAMES)]
        self.param_floats, self.buffer_floats, self.num_counters = 8 * len(NAMES), 0, 0
        self._register_table(lambda name, shape: torch.zeros(shape))
        self.need = {}                         # (batch, training) -> workspace bytes
        self.calls = []

    def _wcache_bytes(self):
        return 64

    def _refresh(self, only):
        self.calls.append(("refresh", only))

    def _workspace_bytes(self, batch, training, mask):
        self.calls.append(("need", batch, training, mask))
        return self.need.get((batch, training), 128)

    def forward_hip(self, batch, training, payload=None):
        mask, ws = self._prepare(batch, training)
        if training:
            self._record_forward(batch, mask, payload)

    def backward_hip(self, d_out, gen):
        B, payload, ws = self._pending(gen, d_out.shape[0])
        self.calls.append(("backward", B, payload, self._same_mask(), gen))

    def refreshes(self):
        out = [c[1] for c in self.calls if c[0] == "refresh"]
        self.calls.clear()
        return out


class _TinyStub(_Hooks, TinyVitBackbone):
    pass


class _ClipStub(_Hooks, _VisionModel):
    pass


STUBS = pytest.mark.parametrize("cls", [_TinyStub, _ClipStub])
d = lambda batch: torch.zeros(batch, 4)


def _refused(rt, text, batch=2, gen=None):
    with pytest.raises(GgError) as e:
        rt.backward_hip(d(batch), rt._gen if gen is None else gen)
    assert str(e.value) == text


@STUBS
def test_every_lifecycle_field_is_declared(cls):
    rt = cls()
    for f in ("_wcache", "_wcache_version", "_synced_ver", "_dirty_all", "_dirty_only", "_ws", "_gen", "_last", "_train_mask", "_last_recompute", "_anchor_t",
              "_grad_ready_hook"):
        assert f in rt.__dict__, f
    assert rt._ws == {} and rt._gen == 0 and rt._last is None and rt._wcache is None and rt._dirty_all is True


@STUBS
def test_workspace_is_reused_regrown_and_released_first(cls, monkeypatch):
    rt = cls()
    rt.need = {(2, True): 256, (1, True): 64, (4, True): 1024, (2, False): 512, (4, False): 2048}
    rt.forward_hip(2, True)
    first = rt._ws[True]
    assert first.numel() == 256 and first.dtype == torch.uint8
    rt.forward_hip(2, True)
    rt.forward_hip(1, True)
    assert rt._ws[True] is first                     # an equal or a smaller need: the same buffer
    rt.forward_hip(2, False)
    assert rt._ws[True] is first and rt._ws[False].numel() == 512 and rt._ws[False] is not first
    # a larger need: the old buffer is gone by the time the new one is asked for
    old, events, empty = weakref.ref(first), rt.calls, torch.empty
    del first
    events.clear()
    monkeypatch.setattr(torch, "empty", lambda n, **kw: (events.append(("alloc", n, old() is None)), empty(n, **kw))[1])
    rt.forward_hip(4, True)
    assert [e[0] for e in events] == ["need", "alloc"] and events[1] == ("alloc", 1024, True)
    assert rt._ws[True].numel() == 1024 and rt._ws[False].numel() == 512          # the two buffers are independent
    kept = rt._ws[True]
    rt.forward_hip(4, False)
    assert rt._ws[False].numel() == 2048 and rt._ws[True] is kept


@STUBS
def test_one_refresh_per_parameter_version_full_or_masked(cls):
    rt = cls()
    rt._ensure_weights()
    assert rt.refreshes() == [None] and rt._wcache.numel() == 64
    rt._ensure_weights()
    rt.forward_hip(2, True)
    assert rt.refreshes() == []
    a, b = bytes([1, 0, 0, 0, 0, 0]), bytes([0, 0, 1, 1, 0, 0])
    rt.mark_params_dirty(only=a)                     # masked raw-pointer writers and nothing else: a masked refresh, the masks OR-ed
    rt.mark_params_dirty(only=b)
    rt._ensure_weights(); rt._ensure_weights()
    assert rt.refreshes() == [bytes([1, 0, 1, 1, 0, 0])]
    rt.mark_params_dirty(only=a)                     # ... with a torch-side write in between: everything
    with torch.no_grad():
        rt._params["head.weight"].add_(1.0)
    rt._ensure_weights(); rt._ensure_weights()
    assert rt.refreshes() == [None]
    rt.mark_params_dirty(only=a)                     # ... with an unmasked mark before or after: everything
    rt.mark_params_dirty()
    rt.mark_params_dirty(only=b)
    rt._ensure_weights()
    assert rt.refreshes() == [None]
    rt.load_state_dict({k: v + 1 for k, v in rt.state_dict().items()})
    rt._ensure_weights(); rt._ensure_weights()
    assert rt.refreshes() == [None]
    rt.mark_params_dirty(only=b)                     # the full refresh above left no stale "everything" behind
    rt._ensure_weights()
    assert rt.refreshes() == [b]


def test_backward_refusals_tinyvit_texts():
    rt = _TinyStub()
    _refused(rt, "TinyViT backward without a training forward")
    rt.forward_hip(2, True, payload="rows")
    rt.forward_hip(2, True, payload="rows")
    _refused(rt, "TinyViT backward for training forward #1, but the workspace now holds the activations of forward #2: saved activations live in ONE "
                 "workspace per backbone, so every training forward must be followed by its backward before the next training forward", gen=1)
    _refused(rt, "TinyViT backward: gradient batch 3 != forward batch 2", batch=3)
    for n in NAMES[1:]:
        rt._params[n].requires_grad = False
    _refused(rt, "requires_grad changed between forward and backward for stem.bias, blocks.0.weight, blocks.0.bias, blocks.1.weight ...: the training "
                 "forward laid out its workspace for the mask it saw (activations only a frozen weight's gradient needs are not kept); run the forward again")
    rt._params["head.weight"].requires_grad = True
    rt._params["blocks.1.weight"].requires_grad = True
    _refused(rt, "requires_grad changed between forward and backward for stem.bias, blocks.0.weight, blocks.0.bias ...: the training "
                 "forward laid out its workspace for the mask it saw (activations only a frozen weight's gradient needs are not kept); run the forward again")
    for n in NAMES:
        rt._params[n].requires_grad = True
    rt.calls.clear()
    rt.backward_hip(d(2), 2)                         # the recorded batch, payload and mask reach the model's backward
    assert rt.calls == [("backward", 2, "rows", bytes([1] * 6), 2)]


def test_backward_refusals_clip_texts():
    rt = _ClipStub()
    _refused(rt, "CLIP backward without a training forward")
    rt.forward_hip(2, True)
    rt.forward_hip(2, True)
    _refused(rt, "CLIP backward for training forward #1, but the workspace now holds the activations of forward #2: every training forward must be "
                 "followed by its backward before the next training forward", gen=1)
    _refused(rt, "CLIP backward: gradient batch 3 != forward batch 2", batch=3)          # (the tower itself passes no batch: its gradients may be None)
    rt._params["stem.bias"].requires_grad = False
    _refused(rt, "requires_grad changed between the CLIP forward and its backward; run the forward again")          # (CLIP's text never named the tensors)
    rt._params["stem.bias"].requires_grad = True
    rt.backward_hip(d(2), 2)


@STUBS
def test_recompute_toggle(cls):
    rt = cls()
    rt.forward_hip(2, True)
    ws = rt._ws[True]
    assert rt.set_recompute(False) is False and rt._ws[True] is ws and rt.cfg.recompute == 0          # the same value: nothing happens
    rt.backward_hip(d(2), 1)
    rt.forward_hip(2, False)
    assert rt.set_recompute(True) is True and rt.cfg.recompute == 1
    assert True not in rt._ws and rt._ws[False] is not None          # the other value: the training workspace (and only it) is released
    tiny = cls is _TinyStub
    assert (rt._last is not None) == tiny
    _refused(rt, "set_grad_checkpointing changed between the training forward and its backward: the forward laid out its workspace for recompute=0 "
                 "(the checkpointed layout keeps other tensors); run the forward again" if tiny else
                 "gradient checkpointing was toggled since the training forward (now recompute=1): its workspace was released, the other layout keeps "
                 "other tensors; run the forward again")
    rt.set_recompute(False)                          # switching back does not revive the forward
    _refused(rt, "TinyViT backward: the training workspace was released (set_grad_checkpointing changed since the training forward); run the forward again"
             if tiny else "gradient checkpointing was toggled since the training forward (now recompute=0): its workspace was released, the other layout "
                          "keeps other tensors; run the forward again")
    rt.set_recompute(True)
    rt.forward_hip(2, True)                          # a new training forward clears the refusal
    assert rt._last_recompute == 1 and rt._ws[True] is not ws
    rt.backward_hip(d(2), 2)


@STUBS
def test_an_eval_forward_leaves_the_training_record_alone(cls):
    rt = cls()
    rt._params["stem.bias"].requires_grad = False
    rt.forward_hip(2, True, payload="rows")
    mask, last, ws = rt._train_mask, rt._last, rt._ws[True]
    assert mask == bytes([1, 0, 1, 1, 1, 1]) and last == (2, "rows", 1)
    rt.calls.clear()
    rt.forward_hip(5, False)
    assert rt.calls == [("need", 5, False, None)]                    # (an eval plan has no mask)
    assert rt._train_mask == mask and rt._last == last and rt._gen == 1 and rt._ws[True] is ws
    rt.backward_hip(d(2), 1)
    assert rt.calls[-1] == ("backward", 2, "rows", mask, 1)


class _Node(EncoderNode):
    @staticmethod
    def forward(ctx, rt, x, anchor, trained):
        rt.forward_hip(x.shape[0], True)
        rt._enter_node(ctx, trained)
        return x * 2


@STUBS
def test_autograd_node_hands_the_generation_to_backward(cls):
    rt = cls()
    assert rt._anchor() is rt._anchor() and rt._anchor().requires_grad and rt._anchor().dim() == 0
    x = torch.ones(3, 4)
    out = _Node.apply(rt, x, rt._anchor(), True)
    rt.calls.clear()
    out.sum().backward()
    assert rt.calls == [("backward", 3, None, bytes([1] * 6), 1)]
    stale = _Node.apply(rt, x, rt._anchor(), True)
    _Node.apply(rt, x, rt._anchor(), True)
    with pytest.raises(GgError, match="for training forward #2, but the workspace now holds the activations of forward #3"):
        stale.sum().backward()
    out = _Node.apply(rt, x, rt._anchor(), False)
    with pytest.raises(GgError) as e:
        out.sum().backward()
    assert str(e.value) == (f"backward through a {rt._name} forward that ran in eval mode (running-stat BatchNorm keeps no activations); "
                            "call .train() before the forward pass")
    assert rt._name == {_TinyStub: "TinyViT", _ClipStub: "CLIP"}[cls]

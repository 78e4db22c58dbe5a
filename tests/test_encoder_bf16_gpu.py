"""GPU: the TPV encoder at the shipped structure (the fixture of tests/test_golden_encoder_full_gpu.py: tests/golden/encoder_full.npz
/ _cfg.json) with the one-product bfloat16 mode of its projections switched on (bricks.LINEAR_BF16).

Routing: with the switch on, every tall-Linear launch of an eval forward and of a forward + backward is a flagged one
(LINEAR_BF16_CALLS equals the launches counted, with the switch off, through a wrapper around the library's linear entry points);
with the switch off the counter stays 0.  The row thresholds are lowered as in that file's `all_kernels` variant, so that on the
fixture's reduced grid every projection takes the HIP route, in every run of this file alike.

Closeness: nobody can derive a bound for the per-plane relative L2 difference from the float32 default run, so the yardstick is a
bf16-Linear model of the same network that exists today: the same encoder under torch.autocast('cuda', dtype=torch.bfloat16) with
the switch off, which rounds operands AND outputs of its Linears.  Its difference from the float32 default run is computed here, on
the same GPU; the switch-on run may differ by at most 2 x that (the two models round at different points, so equal-sized errors can
fall on either side) and must differ by more than 0.  Gradients: the same rule on every parameter gradient of one training step,
the yardstick being a forward + backward under autocast with FUSED_LINEAR_FWD, FUSED_DGRAD and FUSED_WGRAD off.  Those three
switches alone do not make the yardstick a bf16-Linear model: _TallLinear is a custom_fwd(cast_inputs=float32) Function, which
turns autocast OFF inside, so with the row thresholds of this file every projection of the training pass would still be a float32
matmul (measured: such a "yardstick" differs from the float32 run by 3e-7 .. 6e-7, float32 summation noise).  The yardstick run
therefore also raises TallLinear.min_rows, so that every projection is torch's own nn.Linear under autocast — bf16 operands, bf16
outputs, bf16 backward: the model the rule names.
Every figure goes to parity_out/linear_bf16_parity.jsonl (copied to profiles/).

Host syncs: an eval frame and a training step with the switch on run under torch.cuda.set_sync_debug_mode("error")."""
import json
import os

import pytest
import torch

from test_golden_encoder_full_gpu import _setup, _train_pass

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["selfocc_linear_fwd", "selfocc_linear_fwd_heads", "selfocc_linear_fwd_grouped", "selfocc_linear_dgrad",
           "selfocc_linear_dgrad_grouped", "selfocc_linear_wgrad", "selfocc_linear_wgrad_grouped", "selfocc_linear_dgrad_flags",
           "selfocc_linear_dgrad_grouped_flags", "selfocc_linear_wgrad_flags", "selfocc_linear_wgrad_grouped_flags"]
PLANES = ('hw', 'zh', 'wz')


class all_kernels:
    """the row thresholds of test_golden_encoder_full_gpu's `all_kernels` variant (+ the dgrad's), and the switch, for one block"""

    def __init__(self, bf16, tall_min_rows=1, **flags):
        self.bf16, self.tall_min_rows, self.flags = bf16, tall_min_rows, flags

    def __enter__(self):
        from selfocc_amd.model import bricks
        self.old = {k: getattr(bricks, k) for k in ('LINEAR_FWD_MIN_ROWS', 'DGRAD_MIN_ROWS', 'LINEAR_BF16', *self.flags)}
        self.old_min, self.calls = bricks.TallLinear.min_rows, bricks.LINEAR_BF16_CALLS[0]
        bricks.LINEAR_FWD_MIN_ROWS, bricks.DGRAD_MIN_ROWS, bricks.TallLinear.min_rows = 1, 1, self.tall_min_rows
        bricks.LINEAR_BF16 = self.bf16
        for k, v in self.flags.items():
            setattr(bricks, k, v)
        return self

    def flagged(self):
        from selfocc_amd.model import bricks
        return bricks.LINEAR_BF16_CALLS[0] - self.calls

    def __exit__(self, *a):
        from selfocc_amd.model import bricks
        for k, v in self.old.items():
            setattr(bricks, k, v)
        bricks.TallLinear.min_rows = self.old_min
        bricks.LINEAR_BF16_CALLS[0] = self.calls


class count_launches:
    """wrap the library's tall-Linear entry points (the ctypes functions selfocc_amd.linear calls) and count their calls"""

    def __enter__(self):
        from selfocc_amd._lib import lib
        self.l, self.n, self.saved = lib(), {}, {}
        for name in ENTRIES:
            self.saved[name] = getattr(self.l, name)

            def f(*a, _n=name, _f=self.saved[name]):
                self.n[_n] = self.n.get(_n, 0) + 1
                return _f(*a)
            setattr(self.l, name, f)
        return self

    def total(self):
        return sum(self.n.values())

    def __exit__(self, *a):
        for name, f in self.saved.items():
            setattr(self.l, name, f)


def _eval(enc, lifter, feats, metas):
    with torch.no_grad():
        return [o.float() for o in enc(lifter(feats)['representation'], ms_img_feats=feats, metas=metas)['representation']]


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


_WRITTEN = []      # the file is started afresh by the first write of a session, so that a second run does not double its rows


def _write(rows):
    d = os.path.join(ROOT, "parity_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "linear_bf16_parity.jsonl"), "a" if _WRITTEN else "w") as f:
        _WRITTEN.append(len(rows))
        for r in rows:
            f.write(json.dumps(r) + "\n")


@pytest.fixture(scope="module")
def model():
    return _setup()


def test_every_tall_linear_launch_of_the_encoder_is_flagged(hip, model):
    """one eval forward and one forward + backward: launches counted with the switch off == LINEAR_BF16_CALLS with it on; the flagged
    backward entries serve the backward; with the switch off the counter stays 0"""
    z, enc, lifter, feats, metas, loss_dirs = model
    with all_kernels(False) as off, count_launches() as c0:
        _eval(enc, lifter, feats, metas)
        n_eval = c0.total()
        _train_pass(enc, lifter, feats, metas, loss_dirs)
        n_all, names_off = c0.total(), set(c0.n)
        assert off.flagged() == 0
    assert n_eval > 0 and n_all > n_eval and not any(n.endswith("_flags") for n in names_off), c0.n
    with all_kernels(True) as on, count_launches() as c1:
        _eval(enc, lifter, feats, metas)
        assert on.flagged() == c1.total() == n_eval, (on.flagged(), c1.total(), n_eval)
        _train_pass(enc, lifter, feats, metas, loss_dirs)
        assert on.flagged() == c1.total() == n_all, (on.flagged(), c1.total(), n_all)
        # the same launches, the backward ones through the *_flags twins
        assert {n[:-6] if n.endswith("_flags") else n: v for n, v in c1.n.items()} == c0.n, (c0.n, c1.n)
        assert all(n.endswith("_flags") for n in c1.n if "grad" in n), c1.n
    print("tall-Linear launches: eval", n_eval, "eval + training step", n_all, c0.n)


def test_inference_is_as_close_as_the_autocast_encoder(hip, model):
    z, enc, lifter, feats, metas, loss_dirs = model
    with all_kernels(False):
        ref = _eval(enc, lifter, feats, metas)
        assert all(torch.equal(a, b) for a, b in zip(ref, _eval(enc, lifter, feats, metas)))
        with torch.autocast('cuda', dtype=torch.bfloat16):
            amp = _eval(enc, lifter, feats, metas)
    with all_kernels(True) as on:
        got = _eval(enc, lifter, feats, metas)
        assert on.flagged() > 0
    with all_kernels(False):
        assert all(torch.equal(a, b) for a, b in zip(ref, _eval(enc, lifter, feats, metas)))      # the switch leaves nothing behind
    rows = [dict(kind='inference', plane=p, switch_on=rel_l2(g, r), autocast=rel_l2(a, r)) for p, g, a, r in zip(PLANES, got, amp, ref)]
    _write(rows)
    for r in rows:
        print(r)
    for r in rows:
        assert 0.0 < r['switch_on'] <= 2.0 * r['autocast'], r


def test_gradients_are_as_close_as_the_autocast_encoder(hip, model):
    """every parameter gradient of one training step; the yardstick runs under autocast with FUSED_LINEAR_FWD, FUSED_DGRAD and
    FUSED_WGRAD off and every projection on torch's nn.Linear (TallLinear.min_rows raised: see the module docstring)"""
    z, enc, lifter, feats, metas, loss_dirs = model
    with all_kernels(False):
        _, _, ref = _train_pass(enc, lifter, feats, metas, loss_dirs)
    with all_kernels(False, tall_min_rows=1 << 60, FUSED_LINEAR_FWD=False, FUSED_DGRAD=False, FUSED_WGRAD=False):
        with torch.autocast('cuda', dtype=torch.bfloat16):
            _, _, amp = _train_pass(enc, lifter, feats, metas, loss_dirs)
    with all_kernels(True) as on:
        _, _, got = _train_pass(enc, lifter, feats, metas, loss_dirs)
        assert on.flagged() > 0
    rows = [dict(kind='gradient', name='.'.join(k), switch_on=rel_l2(got[k], ref[k]), autocast=rel_l2(amp[k].float(), ref[k]))
            for k in ref if k[0] != 'feat']
    _write(rows)
    worst = sorted(rows, key=lambda r: r['switch_on'] / max(r['autocast'], 1e-30))[-5:]
    for r in worst:
        print(r)
    # One gradient cannot depend on the switch, or on any activation: the bias of the LayerNorm that ends the last layer adds
    # straight into the output, so d loss / d bias is the column sum of the loss direction.  There the difference must be
    # exactly 0 (not "more than 0"); the 2 x rule holds for it like for every other parameter.
    last = f"enc.layers.{len(enc.layers) - 1}.norms.{len(enc.layers[-1].norms) - 1}.bias"
    assert [r['switch_on'] for r in rows if r['name'] == last] == [0.0]
    bad = [r for r in rows if not ((r['name'] == last or 0.0 < r['switch_on']) and r['switch_on'] <= 2.0 * r['autocast'])]
    assert not bad, (len(bad), len(rows), bad[:5])


def test_no_host_sync_with_the_switch_on(hip, model):
    z, enc, lifter, feats, metas, loss_dirs = model
    with all_kernels(True):
        _eval(enc, lifter, feats, metas)                          # first calls: lazy initialisation may synchronise
        _train_pass(enc, lifter, feats, metas, loss_dirs)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = _eval(enc, lifter, feats, metas)
            _, loss, grads = _train_pass(enc, lifter, feats, metas, loss_dirs)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert all(torch.isfinite(o).all().item() for o in out) and torch.isfinite(loss).item()
    assert all(torch.isfinite(g).all().item() for g in grads.values())

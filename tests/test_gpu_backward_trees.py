"""Backward parity past the first level of the reduction trees of kernels_bwd.hip (dw, ln_bwd, the bias-table gradient, the head):
the middle reduce_rows levels, the placement of each level behind the one before, a last group of one row, the split finish after more
than one level and the tree_rows sizing of scratch, dtab and part, at the depths of the training step (B=16 256x256) and of B=16
512x512.  Cases, their row counts and their float64 references: tests/bwd_tree_cases.py (depths, tails and conditioning are held on the
CPU by tests/test_bwd_tree_cases_host.py).

Per case: dense parity (the loss a random linear functional of the outputs; input gradients and every parameter gradient against
torch.autograd of the float64 oracle) and tail-only parity (the upstream gradient zero except the last 16 tokens of the last image,
direct entries the last token: a tree that drops or misplaces its tail returns zero or garbage where the reference has a value), both
under the criteria of tests/test_gpu_backward.py, unchanged.  Two backward calls of the large cases are bit-identical.  The two direct
entries (swf_layernorm_bwd, swf_mlp_bwd through ctypes) always run in a guarded workspace of exactly the queried size with guarded
outputs; one byte less is refused with SWF_ERR_WORKSPACE before anything is launched.  The worst error of every test, in its
criterion's own measure, goes to backward_parity.json next to the parity.json of tests/test_gpu_parity.py."""
import ctypes as C
import faulthandler
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import _lib as L
from swin_unet_image_fusion_amd.modules import _stream
from tests import bwd_tree_cases as BT
from tests.gpu_guard import DEV, Guarded, record_dir

pytestmark = pytest.mark.gpu

_LOG = []   # one record per parity test


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    yield
    if os.environ.get("SWF_PARITY_LOG") == "0":
        return
    out_dir = record_dir()
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "backward_parity.json"), "w") as f:
            json.dump({"metric": "block: max|got-ref| / max(max|ref|, floor), floor 0 for the inputs and 1e-2 gmax for the parameters; model: "
                                 "rel-L2 on the inputs, max|got-ref| / max(max|ref|, 1e-3 gmax) on the parameters; gmax = the largest parameter "
                                 "gradient of the run's own reference; ref = torch.autograd of the CPU oracle in float64; levels = reduce_rows "
                                 "launches of every sum of the case, tree by tree",
                       "gates": {m: {"inputs": b[0], "parameters": b[1]} for m, b in BT.BOUNDS.items()},
                       "records": _LOG}, f, indent=1)
    except OSError:
        pass


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(300, exit=True)   # ends the process when a call does not return
    yield
    faulthandler.cancel_dump_traceback_later()


# ---- one forward and one backward on the GPU ---------------------------------------------------------------------------------------------
def _direct(c, ups, short=False):
    """swf_layernorm_bwd / swf_mlp_bwd through ctypes: workspace of exactly the queried size, gradients in guarded tensors prefilled with
    NaN.  `short`: one byte less, returns (status, outputs untouched).  Otherwise ({"x": gx}, parameter gradients by name)."""
    lib, sd = L.lib(), {k: v.to(DEV) for k, v in BT.state(c).items()}
    x, gout = BT.inputs(c)[0].to(DEV), ups[0].to(DEV).contiguous()
    n = c.N
    gx = Guarded((n, c.C))
    if c.kind == "layernorm":
        names = ("norm_layer_1.weight", "norm_layer_1.bias")
        need = lib.swf_layernorm_bwd_workspace_bytes(n, c.C)
    else:
        names = ("mlp_x_1.weight", "mlp_x_1.bias", "mlp_x_2.weight", "mlp_x_2.bias")
        need = lib.swf_mlp_bwd_workspace_bytes(n, c.C, c.hidden)
    grads = {k: Guarded(tuple(sd[k].shape)) for k in names}
    ws = Guarded((need,), torch.uint8)
    for g in [gx] + list(grads.values()):
        g.t.fill_(float("nan"))
    room = need - 1 if short else need
    p = lambda k: sd[k].data_ptr()
    g = lambda k: grads[k].t.data_ptr()
    if c.kind == "layernorm":
        ln, gp = L.Norm(p(names[0]), p(names[1])), L.Norm(g(names[0]), g(names[1]))
        st = lib.swf_layernorm_bwd(C.byref(ln), x.data_ptr(), gout.data_ptr(), gx.t.data_ptr(), C.byref(gp), n, c.C, ws.t.data_ptr(), room,
                                   _stream(x.device))
    else:
        f1, f2 = L.Linear(p(names[0]), p(names[1])), L.Linear(p(names[2]), p(names[3]))
        g1, g2 = L.Linear(g(names[0]), g(names[1])), L.Linear(g(names[2]), g(names[3]))
        st = lib.swf_mlp_bwd(C.byref(f1), C.byref(f2), x.data_ptr(), gout.data_ptr(), gx.t.data_ptr(), C.byref(g1), C.byref(g2), n, c.C, c.hidden,
                             ws.t.data_ptr(), room, _stream(x.device))
    torch.cuda.synchronize()
    guarded = [gx, ws] + list(grads.values())
    assert all(t.intact() for t in guarded), "an entry wrote outside a guarded tensor or its workspace"
    if short:
        return st, [t.t for t in [gx] + list(grads.values())]
    assert st == L.OK, lib.swf_last_error_string()
    return {"x": gx.t.clone()}, {k: v.t.clone() for k, v in grads.items()}


def _masks_are_the_restatement(c, seed):
    """swf_dropout_mask with the block's own seed gives exactly the factors the reference was computed with"""
    assert seed == BT.drop_seed(c), (seed, BT.drop_seed(c))
    ref, n = BT.drop_masks(c), c.B * c.H * c.W
    for s in (0, 1):
        for site, wd in enumerate(BT.DROP_SITE_WIDTHS(c)):
            out = torch.empty(n * wd, dtype=torch.float32, device=DEV)
            L.check(L.lib().swf_dropout_mask(seed, s, site, n * wd, c.drop, out.data_ptr(), _stream(out.device)))
            want = ref(s, site, wd).permute(0, 2, 3, 1).reshape(-1).numpy()
            assert np.array_equal(out.cpu().numpy(), want), (s, site)


def _run(c, mode, ref=None):
    """(input gradients, parameter gradients) by name of one forward + backward of the case on the GPU; with `ref` the forward's outputs
    (head, model) and the head's running statistics are held to the reference's as tests/test_gpu_backward.py holds them."""
    ups = BT.upstream(c, mode)
    if c.direct:
        return _direct(c, ups)
    m = BT.make_module(c).to(DEV)
    names = BT.param_names(c)
    params = dict(m.named_parameters())
    if c.kind == "block":
        m.precision = "fp32"
    if c.kind == "model" or (c.kind == "block" and c.drop) or (c.kind == "head" and c.train):
        m.train()
    ins = [t.to(DEV).requires_grad_(True) for t in BT.inputs(c)]
    if c.kind == "block" and c.drop:
        torch.manual_seed(c.seed)
    if c.kind == "attention":
        outs = [m(ins[0], ins[1], ins[1])]
    elif c.kind == "head":
        outs = [m.do_final_layer(*ins)]
    else:
        outs = m(*ins)
        outs = list(outs) if isinstance(outs, tuple) else [outs]
    assert all(o.requires_grad for o in outs)
    if c.kind == "block" and c.drop:
        _masks_are_the_restatement(c, m.last_dropout_seed)
    if ref is not None and c.kind == "head":
        assert torch.allclose(outs[0].detach().cpu(), ref["out"][0].float(), rtol=1e-4, atol=1e-5)
        bn = m.final_layer[1]
        for k, got in (("final_layer.1.running_mean", bn.running_mean), ("final_layer.1.running_var", bn.running_var)):
            assert torch.allclose(got.cpu(), ref["running"][k].float(), rtol=1e-5, atol=1e-6), (k, got.cpu(), ref["running"][k])
            assert torch.equal(got.cpu(), BT.state(c)[k]) != c.train, k       # moved by the batch statistics in train(), kept in eval()
    if ref is not None and c.kind in ("model", "attention"):
        o, r = outs[0].detach().cpu().double(), ref["out"][0]
        assert float((o - r).abs().max() / r.abs().max()) <= 2e-3
    gs = torch.autograd.grad(outs, ins + [params[k] for k in names], [u.to(DEV) for u in ups])
    assert len(names) == (len(params) if c.kind != "head" else 6)
    return dict(zip(BT.INPUT_NAMES[c.kind], gs[:len(ins)])), dict(zip(names, gs[len(ins):]))


def _parity(c, mode):
    ref = BT.reference64(c)
    got_in, got_par = _run(c, mode, ref)
    for t in list(got_in.values()) + list(got_par.values()):
        assert bool(torch.isfinite(t).all())
    e_in, e_par, which = BT.measure(c.metric, got_in, got_par, *ref[mode])
    b_in, b_par = BT.BOUNDS[c.metric]
    print(f"[bwd-trees] {c.id} {mode}: inputs {e_in:.3e} (bound {b_in:.0e}) parameters {e_par:.3e} at {which} (bound {b_par:.0e})")
    _LOG.append({"case": c.id, "mode": mode, "metric": c.metric, "levels": {t: list(v) for t, v in c.depth}, "inputs": e_in, "parameters": e_par,
                 "worst_parameter": which, "passed": bool(e_in <= b_in and e_par <= b_par)})
    assert e_in <= b_in, (c.id, mode, "inputs", e_in)
    assert e_par <= b_par, (c.id, mode, which, e_par)


@pytest.mark.parametrize("case", BT.CASES, ids=lambda c: c.id)
def test_dense_parity_vs_autograd_of_the_oracle(case):
    _parity(case, "dense")


@pytest.mark.parametrize("case", BT.CASES, ids=lambda c: c.id)
def test_tail_only_parity_vs_autograd_of_the_oracle(case):
    _parity(case, "tail")


@pytest.mark.parametrize("case", BT.BIT_REPRODUCIBLE, ids=lambda c: c.id)
def test_two_backward_calls_are_bit_identical(case):
    """Every level of every tree sums in index order, without atomics."""
    runs = [_run(case, "dense") for _ in range(2)]
    for a, b in zip(*runs):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("case", BT.DIRECT, ids=lambda c: c.id)
def test_direct_entry_refuses_a_workspace_one_byte_short(case):
    st, outs = _direct(case, BT.upstream(case, "dense"), short=True)
    assert st == L.ERR_WORKSPACE, (st, L.lib().swf_last_error_string())
    assert all(bool(torch.isnan(t).all()) for t in outs), "the entry launched before it checked its workspace"

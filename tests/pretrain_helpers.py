"""Shared by test_pretrain_cpu.py and test_gpu_pretrain.py: the targets of the pretraining tests and the loss of reference
pretrain.py:70-94 with torch autograd over the oracle's `eval_mats` (the role jax.value_and_grad plays at pretrain.py:91)."""
import contextlib

import numpy as np
import torch

from common import oracle_net
from oracle.network import params_to_torch, working_dtype

# cases of tests/golden/pretrain.npz (tools/make_pretrain_golden.py): names of oracle.testing.CASES
GOLDEN_CASES = ('lih', 'lih_twist', 'bcc_li', 'lih_fulldet', 'lih_lastlayer', 'lih_bias', 'lih_fn_defaults')


def plane_waves(klist, x):
    """exp(i k_m . r_i) per spin, numpy: x (B, 3N) -> [(B, n_s, n_s) complex128 for every spin with electrons]."""
    x = np.asarray(x, dtype=np.float64).reshape(len(x), -1, 3)
    out, i0 = [], 0
    for k in klist:
        k = np.asarray(k, dtype=np.float64).reshape(-1, 3)
        if k.shape[0]:
            out.append(np.exp(1j * np.einsum('bic,mc->bim', x[:, i0:i0 + k.shape[0]], k)))
        i0 += k.shape[0]
    return out


def make_targets(klist, x, seed, rel=0.1):
    """Plane-wave targets plus a seeded complex perturbation of relative size `rel` (|plane wave| = 1 for a real k): no
    structure of the target is relied on."""
    rng = np.random.default_rng(seed)
    return [t + rel * (rng.normal(size=t.shape) + 1j * rng.normal(size=t.shape)) for t in plane_waves(klist, x)]


def reference_loss(predict, target, full_det):
    """pretrain.py:78-88 on torch values: predict = list of (B, n_det, n, n), target = list of (B, n_s, n_s)."""
    if full_det:
        B, na, nb = predict[0].shape[0], target[0].shape[1], target[1].shape[1] if len(target) > 1 else 0
        up = torch.cat([target[0], torch.zeros(B, na, nb, dtype=target[0].dtype)], dim=-1)
        if nb:
            up = torch.cat([up, torch.cat([torch.zeros(B, nb, na, dtype=target[0].dtype), target[1]], dim=-1)], dim=-2)
        target = [up]
    return torch.stack([((tar[:, None] - pre).abs() ** 2).mean() for tar, pre in zip(target, predict)]).mean()


def oracle_pretrain(cell, klist, net_kw, params, x, targets, dtype=None):
    """-> (loss float, gradient tree shaped like params) of the pretraining loss at walkers x (B, 3N), from autograd over the
    oracle.  dtype=torch.float32: parameters, walkers, targets and the restated forward in float32 / complex64."""
    ctx = working_dtype(dtype) if dtype is not None else contextlib.nullcontext()
    with ctx:
        net = oracle_net(cell, klist, net_kw, 'eval_mats')
        rd = dtype or torch.float64
        cd = torch.complex64 if rd == torch.float32 else torch.complex128
        x = torch.as_tensor(np.asarray(x)).to(rd)
        tg = [torch.as_tensor(np.asarray(t)).to(cd) for t in targets]
        lv = []

        def req(o):
            if isinstance(o, dict):
                return {k: req(v) for k, v in o.items()}
            if isinstance(o, (list, tuple)):
                return [req(v) for v in o]
            t = o.clone().detach().requires_grad_(True)
            lv.append(t)
            return t
        p = req(params_to_torch(params, dtype))
        per_walker = [net.apply(p, xx) for xx in x]                       # vmap over the batch
        predict = [torch.stack([m[c] for m in per_walker]) for c in range(len(per_walker[0]))]
        loss = reference_loss(predict, tg, bool(net_kw.get('full_det', False)))
        grads = iter(torch.autograd.grad(loss, lv, allow_unused=True))

        def build(o):
            if isinstance(o, dict):
                return {k: build(v) for k, v in o.items()}
            if isinstance(o, (list, tuple)):
                return [build(v) for v in o]
            g = next(grads)
            return torch.zeros_like(o) if g is None else g
        return float(loss.detach()), build(p)


def leaves(tree):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from leaves(tree[k])
    elif isinstance(tree, (list, tuple)):
        for v in tree:
            yield from leaves(v)
    else:
        yield tree


def leaf_names(tree, path=()):
    """Leaf names in the order of `leaves` ('single/0/w', ...): the keys of tests/golden/pretrain.npz."""
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from leaf_names(tree[k], path + (k,))
    elif isinstance(tree, (list, tuple)):
        for i, v in enumerate(tree):
            yield from leaf_names(v, path + (i,))
    else:
        yield '/'.join(str(q) for q in path)


def leaf_devs(got, ref):
    """Per leaf: max |got - ref| / max |ref|."""
    out = []
    for g, r in zip(leaves(got), leaves(ref)):
        g = g.detach().double().cpu().numpy()
        r = r.detach().double().cpu().numpy() if isinstance(r, torch.Tensor) else np.asarray(r, dtype=np.float64)
        assert g.shape == r.shape
        out.append(float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-300)))
    return out


def check_against_fixture(fx, name, loss, grad_tree, params):
    """The reference-executed numbers of tests/golden/pretrain.npz for case `name` against (loss, gradient tree): loss to 1e-10
    relative; per-leaf norms, projections on make_test_direction and the leaves stored element-wise to 1e-8 of the largest
    leaf norm (the bounds of test_energy_gradient_vs_reference_train).  -> (loss deviation, worst gradient deviation), relative."""
    from oracle.testing import make_test_direction
    pre = name + ':'
    vdir = list(leaves(make_test_direction(int(fx[pre + 'seed']), params)))
    gl = [g.detach().double().cpu().numpy() for g in leaves(grad_tree)]
    names = list(leaf_names(params))
    assert names == [str(n) for n in fx[pre + 'names']]
    ref_loss = float(fx[pre + 'loss'])
    dl = abs(loss - ref_loss) / abs(ref_loss)
    scale = float(np.max(fx[pre + 'norm']))
    worst = 0.0
    for i, (n, g) in enumerate(zip(names, gl)):
        worst = max(worst, abs(np.linalg.norm(g) - fx[pre + 'norm'][i]) / scale,
                    abs(float((g * vdir[i]).sum()) - fx[pre + 'dot'][i]) / scale)
        if pre + 'leaf:' + n in fx:
            worst = max(worst, float(np.abs(g - fx[pre + 'leaf:' + n]).max()) / scale)
    assert dl <= 1e-10, (name, loss, ref_loss)
    assert worst <= 1e-8, (name, worst)
    return dl, worst

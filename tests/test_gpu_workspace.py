"""Canary tests of the workspace layouts of the host code (csrc/ds_host.h and the units over it): every entry point that carves a caller-supplied workspace is run in
a buffer of exactly the size the library reports, followed by 1 MiB of 0xA5 inside the same torch allocation.  A carve that hands
out more than the size function counted overwrites the canary and shows as a failed assertion (not as a memory fault); the
result must equal the same call in the cached, uncapped workspace:

* bit for bit for `logpsi`, `logpsi_grad`, `local_energy` and the four fused samplers (their chunking never changes a walker's
  arithmetic);
* for the three gradient passes to the bound of their own chunk tests (test_vjp_groups_chunks_and_linearity,
  test_pretrain_chunks_..., test_two_calls_same_bits_chunks_agree_...): 1e-12 of each leaf's / factor's largest entry in float64 --
  about 4500 float64 round-offs -- and the same number of float32 round-offs (1e-12 * 2^29) in float32.

Cells: the small fixtures that reach each branch of the layouts (plain, use_last_layer, one spin channel, one dense determinant
channel, unequal padded widths, orbital bias, more than one slot tile -- the last in float32 too).  Batches: one walker, 83 (two
groups of 80, the second ragged) and, for the gradient passes, 163 walkers in a one-group workspace (three passes)."""
import numpy as np
import pytest
import torch

import sampler_helpers as sh
from common import load_case
from deepsolid_amd import systems
from deepsolid_amd.device import DeviceSystem, _ptr, _stream
from pretrain_helpers import make_targets

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
CELLS = [('lih', F64), ('lih_lastlayer', F64), ('li_polarized', F64), ('lih_fulldet', F64), ('lih_mixed', F64), ('lih_bias', F64),
         ('bcc_li', F64), ('bcc_li', F32)]
IDS = [f'{n}-{"f64" if d == F64 else "f32"}' for n, d in CELLS]
TAIL = 1 << 20
CANARY = 0xA5
CHUNK_TOL = {F64: 1e-12, F32: 1e-12 * 2 ** 29}


def case_system(name, dtype):
    """-> (system, device parameters, cell, klist)."""
    _, cell, klist, net_kw, params = load_case(name)
    sysd = DeviceSystem.for_network(cell, klist, net_kw, dtype)
    dp = {k: [{kk: torch.as_tensor(np.asarray(vv), dtype=dtype, device='cuda') for kk, vv in d.items()} for d in v]
          for k, v in params.items()}
    return sysd, dp, cell, klist


def walkers(cell, B, dtype):
    return torch.as_tensor(systems.synthetic_walkers(cell, B, seed=29), dtype=dtype, device='cuda')


class Canary:
    """`sysd._ws` = `need` bytes for the call + TAIL bytes of CANARY; `check()` after the call."""

    def __init__(self, sysd, need):
        assert need > 0
        self.sysd, self.need = sysd, need
        self.buf = torch.full((need + TAIL,), CANARY, dtype=torch.uint8, device='cuda')
        sysd._ws = self.buf

    def check(self):
        torch.cuda.synchronize()
        assert self.sysd._ws is self.buf, 'the call replaced the workspace: it asked for more than the size it reported'
        tail = self.buf[self.need:]
        bad = int((tail != CANARY).sum())
        first = int((tail != CANARY).nonzero()[0]) if bad else -1
        self.sysd._ws = None
        assert bad == 0, f'{bad} bytes written behind a workspace of {self.need} bytes (first at +{first})'


def flat(out):
    """Every tensor of a (nested) result, None dropped."""
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out]
    return [t for o in out for t in flat(o)]


def assert_same_bits(got, ref):
    got, ref = flat(got), flat(ref)
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert g.shape == r.shape and torch.equal(g, r), float((g - r).abs().max())


def assert_close(got, ref, tol):
    """max |got - ref| <= tol * max |ref| per tensor (0-d tensors: relative)."""
    got, ref = flat(got), flat(ref)
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert g.shape == r.shape
        dev, scale = float((g - r).abs().max()), float(r.abs().max())
        assert dev <= tol * scale, (tuple(g.shape), dev, scale, tol)


@pytest.mark.parametrize('method', ['local_energy', 'logpsi', 'logpsi_grad'])
@pytest.mark.parametrize('name,dtype', CELLS, ids=IDS)
def test_energy_path_stays_inside_the_reported_workspace(name, dtype, method):
    sysd, dp, cell, _ = case_system(name, dtype)
    kw = dict(want_logpsi=True) if method == 'local_energy' else {}
    for B in (1, 83):
        x = walkers(cell, B, dtype)
        sysd._ws = None
        ref = [t.clone() for t in flat(getattr(sysd, method)(dp, x, **kw))]
        need = int(sysd.lib.ds_workspace_bytes(sysd.handle, B))
        can = Canary(sysd, need)
        got = getattr(sysd, method)(dp, x, ws_bytes=need, **kw)
        can.check()
        assert_same_bits(got, ref)


def grad_call(sysd, method, dp, x, klist, **kw):
    """-> the result of gradient pass `method`, the packed gradient unpacked so that the tolerance applies per leaf / per factor."""
    B = x.shape[0]
    if method == 'logpsi_vjp':
        cot = torch.as_tensor(np.random.default_rng(9).normal(size=(B, 2)), dtype=sysd.dtype, device='cuda')
        g, la, ph = sysd.logpsi_vjp(dp, x, cot, **kw)
        return [sysd.unpack_grad(g.clone(), dp), la.clone(), ph.clone()]
    if method == 'pretrain_loss_vjp':
        cd = torch.complex128 if sysd.dtype == F64 else torch.complex64
        targets = [torch.as_tensor(t, dtype=cd, device='cuda') for t in make_targets(klist, x.double().cpu().numpy(), 11)]
        loss, g = sysd.pretrain_loss_vjp(dp, x, targets, **kw)
        return [loss.clone(), sysd.unpack_grad(g.clone(), dp)]
    fac, g = sysd.kfac_factors(dp, x, **kw)
    return [[(A.clone(), G.clone()) for A, G in fac], sysd.unpack_grad(g.clone(), dp)]


def leaves(tree):
    if isinstance(tree, dict):
        return [t for k in sorted(tree) for t in leaves(tree[k])]
    if isinstance(tree, (list, tuple)):
        return [t for v in tree for t in leaves(v)]
    return [tree]


SIZE_FN = {'logpsi_vjp': 'ds_vjp_workspace_bytes', 'pretrain_loss_vjp': 'ds_pretrain_workspace_bytes',
           'kfac_factors': 'ds_kfac_workspace_bytes'}


@pytest.mark.parametrize('method', sorted(SIZE_FN))
@pytest.mark.parametrize('name,dtype', CELLS, ids=IDS)
def test_gradient_passes_stay_inside_the_reported_workspace(name, dtype, method):
    sysd, dp, cell, klist = case_system(name, dtype)
    size = getattr(sysd.lib, SIZE_FN[method])
    for B, cap_batch in ((1, 1), (83, 83), (163, 1)):       # (163, 1): a one-group workspace, three passes
        x = walkers(cell, B, dtype)
        sysd._ws = None
        ref = grad_call(sysd, method, dp, x, klist)
        need = int(size(sysd.handle, cap_batch))
        assert need > 0
        if cap_batch < B:
            assert need < int(size(sysd.handle, B))
        can = Canary(sysd, need)
        got = grad_call(sysd, method, dp, x, klist, max_bytes=need)
        can.check()
        assert_close(leaves(got), leaves(ref), CHUNK_TOL[dtype])


def sampler_call(sysd, kind, p, x, lp, steps, width, seed, atoms, ws, ws_bytes):
    """The C entry point of sampler `kind` itself (`DeviceSystem.mcmc_step` always passes its whole cached buffer)."""
    from deepsolid_amd import _lib
    B = x.shape[0]
    nacc = torch.zeros(1, dtype=sysd.dtype, device='cuda')
    head = (sysd.handle, _ptr(p), _ptr(x), _ptr(lp), B, steps)
    tail = (seed, 0, _ptr(None), _ptr(None), 0, _ptr(nacc), _ptr(ws), ws_bytes, _stream())
    if kind == 'mh':
        rc = sysd.lib.ds_mcmc_step(*head, float(width), *tail)
    elif kind == 'one':
        rc = sysd.lib.ds_mcmc_step_one_electron(*head, 1, float(width), *tail)
    elif kind == 'imp':
        rc = sysd.lib.ds_mcmc_step_importance(*head, float(width), *tail)
    else:
        rc = sysd.lib.ds_mcmc_step_asymmetric(*head, float(width), _ptr(atoms), int(atoms.shape[0]), *tail)
    _lib.check(rc, 'sampler ' + kind)
    return nacc


@pytest.mark.parametrize('kind', ['mh', 'one', 'imp', 'asym'])
@pytest.mark.parametrize('name,dtype', CELLS, ids=IDS)
def test_samplers_stay_inside_the_reported_workspace(name, dtype, kind):
    sysd, dp, cell, _ = case_system(name, dtype)
    atoms = torch.as_tensor(sh.nuclei(cell), dtype=dtype, device='cuda').contiguous()
    width = {'mh': 0.05, 'one': 0.5, 'imp': 0.05, 'asym': 0.02}[kind]
    kw = {'mh': {}, 'one': dict(first_electron=1), 'imp': dict(importance=True), 'asym': dict(atoms=atoms)}[kind]
    for B in (1, 83):
        x0 = walkers(cell, B, dtype)
        sysd._ws = None
        xr, lpr = x0.clone(), torch.empty(B, dtype=dtype, device='cuda')
        nr = sysd.mcmc_step(dp, xr, lpr, 2, width, seed=5, **kw)
        p = sysd.pack_params(dp)
        need = int(sysd.lib.ds_mcmc_workspace_bytes(sysd.handle, B))
        can = Canary(sysd, need)
        x, lp = x0.clone(), torch.empty(B, dtype=dtype, device='cuda')
        n = sampler_call(sysd, kind, p, x, lp, 2, width, 5, atoms, can.buf, need)
        can.check()
        assert_same_bits([x, lp, n], [xr, lpr, nr])


@pytest.mark.parametrize('name', ['lih_plain', 'lih_last_bias', 'li_polarized'])
def test_header_block_rule_is_the_library_layout(name):
    """The blocks tests/test_params_cpu.py lays out by the rule of include/deepsolid_hip.h are `ds_param_layout` of a real handle,
    element count included; the buffer packed on the device is the one the CPU map packs."""
    import param_map_helpers as pmh
    cell, klist, net_kw = pmh.case_net(name)
    for dtype in (F64, F32):
        sysd = DeviceSystem.for_network(cell, klist, net_kw, dtype)
        pm, _, _ = pmh.param_map(name, dtype)
        assert sysd.blocks == pm.blocks and sysd.param_count == pm.param_count
        tree = pmh.make_tree(cell, net_kw, dtype=dtype)
        assert np.array_equal(sysd.param_map.layout(tree).gather, pm.layout(tree).gather)
        dp = {k: [{kk: vv.cuda() for kk, vv in d.items()} for d in v] for k, v in tree.items()}
        assert torch.equal(sysd.pack_params(dp).cpu(), pm.pack(tree, 'cpu', dtype))

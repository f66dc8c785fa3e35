"""DeviceSystem: one simulation cell + network architecture resident on one GPU.

Owns the C-ABI handle (``ds_system``), the packed parameter buffer and the
scratch workspace; every numeric call of the package ends in one of the
``ds_*`` entry points of libdeepsolid_hip.so here.  Walkers, parameters and
results are torch tensors on the ROCm device -- torch is used for memory,
streams and (elsewhere) torch.distributed, nothing else.
"""
import ctypes as C
import re
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .params import ParamMap

_DTYPES = {torch.float64: 0, torch.float32: 1}
OBDM_GROUP = 128        # ds::OBDM_GROUP of csrc/ds_obdm.h: samples per partial row of ds_obdm_accumulate (chunks are whole groups)


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _DmcVariant(NamedTuple):
    """One of the three step entries behind `DeviceSystem.dmc_step`.  noise: the explicit noise arrays in the entry's order, each
    (keyword, float64 (else the system's dtype), shape behind the leading `steps` as a function of (B, 3N)); lead: the entries of
    rotations and pairs that an initialisation takes; columns: of ecp_stats."""
    entry: str
    ws_entry: str
    noise: tuple
    lead: int
    columns: int
    noise_message: str


_DMC_NOISE = (('normals', False, lambda B, n3: (B, n3)), ('uniforms', False, lambda B, n3: (B,)), ('comb_uniforms', True, lambda B, n3: ()))
_DMC_ROTATIONS = ('rotations', True, lambda B, n3: (B, 3, 3))
_DMC_MESSAGE = 'explicit noise must be normals (steps, B, 3N), uniforms (steps, B)'
_DMC_VARIANTS = dict(
    plain=_DmcVariant('ds_dmc_step', 'ds_dmc_workspace_bytes', _DMC_NOISE, 0, 0, _DMC_MESSAGE + ' and comb_uniforms (steps,)'),
    ecp=_DmcVariant('ds_dmc_step_ecp', 'ds_dmc_ecp_workspace_bytes', _DMC_NOISE + (_DMC_ROTATIONS,), 1, 3,
                    _DMC_MESSAGE + ', comb_uniforms (steps,) and rotations (steps + 1, B, 3, 3)'),
    tmove=_DmcVariant('ds_dmc_step_tmove', 'ds_dmc_tmove_workspace_bytes',
                      _DMC_NOISE + (_DMC_ROTATIONS, ('tmove_uniforms', True, lambda B, n3: (B,))), 0, 4,
                      _DMC_MESSAGE + ', comb_uniforms (steps,) and rotations (steps, B, 3, 3)'))


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError('deepsolid_amd needs a ROCm GPU: there is no CPU path (the CPU oracle lives in '
                           'oracle/ and is test infrastructure only)')


def device_plan(hidden_dims, n_in_single, n_in_double=4, n_double=None):
    """-> (device widths, residual flags) for the reference's `hidden_dims` (network.py:111-132), from the library itself
    (`ds_device_widths`: host code of the C ABI, no GPU needed; `ds_system_create` applies the same plan to its descriptor).

    The kernels run one-electron widths in multiples of 64 and pair widths of 16 or 32; any other width runs with ZERO-PADDED
    weights and biases, which is exact: a padded feature is tanh(0) = 0 in every layer, has zero jets, adds nothing to the spin
    means and meets zero rows in the next layer.  A residual is added exactly where the reference adds one (network.py:525-528:
    in == out of the REFERENCE's widths) -- an explicit flag per layer and stream, independent of the padded widths.
    `n_in_single` / `n_in_double`: widths of the input features (nf x atoms, nf); `n_double`: number of pair layers that run
    (network.py:118-121: the last width is unused without `use_last_layer`).  Raises ValueError for what the kernels cannot run:
    widths beyond 1024 / 32.  A first layer as wide as its input features (either stream: the reference's residual there) runs for
    any width: the residual is added behind the layer."""
    import ctypes as C
    lib = _lib.load()
    n = len(hidden_dims)
    n_double = n if n_double is None else n_double
    arr = C.c_int32 * max(n, 1)
    hs, hd = arr(*[int(h[0]) for h in hidden_dims]), arr(*[int(h[1]) for h in hidden_dims])
    ps, pd, rs, rd = arr(), arr(), arr(), arr()
    if lib.ds_device_widths(hs, hd, n, int(n_in_single), int(n_in_double), int(n_double), ps, pd, rs, rd) != 0:
        raise ValueError(lib.ds_last_error().decode())
    return tuple(zip(ps[:n], pd[:n])), tuple(zip((bool(v) for v in rs[:n]), (bool(v) for v in rd[:n])))


def device_widths(hidden_dims, n_in_single, n_double=None, n_in_double=4):
    """The widths the kernels run for the reference's `hidden_dims` (see `device_plan`)."""
    return device_plan(hidden_dims, n_in_single, n_in_double, n_double)[0]


class DeviceSystem:
    def __init__(self, simulation_cell, klist, net_kw, tables, dtype=torch.float64, device=None):
        _require_gpu()
        self.lib = _lib.load()
        self.cell = simulation_cell
        self.dtype = dtype
        self.device = torch.device(device if device is not None else f'cuda:{torch.cuda.current_device()}')
        self.net_kw = dict(net_kw)
        self.tables = tables
        prim = simulation_cell.original_cell
        self.nelec = tuple(int(n) for n in simulation_cell.nelec)
        if self.nelec[0] == 0 and self.nelec[1] > 0:
            # only spin-down electrons -- an EXTENSION beyond the reference: its parameter tree drops the empty channel
            # (network.py:113-117) but its forward then raises (network.py:537-553 pairs the empty block with orbital[0]).  The
            # parameter tree is that of the mirrored cell (n_dn, 0), which is what runs here; the library does the same swap for a
            # C caller.  Checked against this repo's oracle only, not against reference-executed numbers
            self.nelec = (self.nelec[1], 0)
            klist = (klist[1], klist[0])
        self.n = sum(self.nelec)
        self.n_det = int(net_kw['determinants'])
        self.hidden_dims = tuple(tuple(int(v) for v in h) for h in net_kw['hidden_dims'])
        nf = 4 if net_kw.get('distance_type', 'nu') == 'nu' else 7
        nf_in = nf * np.asarray(prim.atom_coords()).reshape(-1, 3).shape[0]
        # what the kernels run (zero-padded weights) and where a residual is added: the library's own plan; the descriptor below
        # carries the REFERENCE's widths, ds_system_create pads them the same way
        self.device_dims, self.residuals = device_plan(self.hidden_dims, nf_in, nf,
                                                       len(self.hidden_dims) - (0 if net_kw.get('use_last_layer', False) else 1))
        d = _lib.SystemDesc()
        keep = []                       # host arrays must outlive ds_system_create

        def arr(a):
            a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
            keep.append(a)
            return _pd(a)
        d.dtype = _DTYPES[dtype]
        d.n_up, d.n_dn = self.nelec
        atoms = np.asarray(prim.atom_coords(), dtype=np.float64).reshape(-1, 3)
        d.n_atoms_prim = atoms.shape[0]
        self.n_atoms_prim = int(atoms.shape[0])
        self.prim_atoms = atoms.copy()
        d.prim_atoms = arr(atoms)
        d.prim_a[:] = np.asarray(prim.a, dtype=np.float64).reshape(-1).tolist()
        d.sim_a[:] = np.asarray(simulation_cell.a, dtype=np.float64).reshape(-1).tolist()
        n_sym = np.asarray(simulation_cell.AV).shape[0]
        d.n_sym = n_sym
        for name, src in (('prim_AV', prim.AV), ('prim_BV', prim.BV), ('sim_AV', simulation_cell.AV),
                          ('sim_BV', simulation_cell.BV)):
            flat = np.zeros(_lib.DS_MAX_SYM * 3)
            flat[:3 * n_sym] = np.asarray(src, dtype=np.float64).reshape(-1)
            getattr(d, name)[:] = flat.tolist()
        d.n_layers = len(self.hidden_dims)
        for i, (a, b) in enumerate(self.hidden_dims):
            d.hidden_single[i], d.hidden_double[i] = a, b
        d.n_det = self.n_det
        d.distance_type = {'nu': 0, 'tri': 1}.get(net_kw.get('distance_type', 'nu'), 99)
        d.envelope_type = {'isotropic': 0, 'diagonal': 1, 'full': 2}.get(net_kw.get('envelope_type'), 99)
        d.full_det = int(bool(net_kw.get('full_det', False)))
        d.use_last_layer = int(bool(net_kw.get('use_last_layer', False)))
        d.bias_orbitals = int(bool(net_kw.get('bias_orbitals', False)))
        kl = [np.asarray(k, dtype=np.float64).reshape(-1, 3) for k in klist]
        if kl[0].shape[0] != self.nelec[0] or kl[1].shape[0] != self.nelec[1]:
            raise ValueError('klist must hold one k vector per electron of each spin (hf.py:99-104)')
        d.klist_up, d.klist_dn = arr(kl[0]), arr(kl[1] if kl[1].size else np.zeros((1, 3)))
        t = tables
        d.n_atoms_sim = t.atom_coords.shape[0]
        d.sim_atoms, d.sim_charges = arr(t.atom_coords), arr(t.atom_charges)
        d.dist_mode = t.dist_mode
        d.n_g = t.gpoints.shape[0]
        d.gpoints, d.gweight = arr(t.gpoints), arr(t.gweight)
        d.ion_exp_re, d.ion_exp_im = arr(t.ion_exp.real), arr(t.ion_exp.imag)
        d.ewald_alpha = float(t.alpha)
        d.ee_const, d.ei_const = float(t.ee_const(self.n)), float(t.ei_const(self.n))
        d.ii_total = float(t.ion_ion + t.ii_const)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ds_system_create(C.byref(d), C.byref(handle)), 'ds_system_create')
        self.handle = handle
        nb = self.lib.ds_param_layout(handle, None, 0)
        blocks = (_lib.ParamBlock * nb)()
        self.lib.ds_param_layout(handle, blocks, nb)
        self.blocks = [(int(b.offset), int(b.rows), int(b.cols)) for b in blocks]
        self.param_count = int(self.lib.ds_param_count(handle))
        # the tree <-> buffer index map, the packed-buffer cache and the KFAC index live there
        self.param_map = ParamMap(self.nelec, self.n_det, self.hidden_dims, self.device_dims, atoms.shape[0],
                                  net_kw.get('distance_type', 'nu'), net_kw.get('envelope_type'), d.full_det, d.use_last_layer,
                                  d.bias_orbitals, dtype, self.blocks, self.param_count)
        self._ws = None

    # ------------------------------------------------------------------ construction helpers
    @classmethod
    def for_network(cls, simulation_cell, klist, net_kw, dtype=torch.float64):
        from .ewaldsum import EwaldTables
        key = ('net', id(simulation_cell), dtype, repr(sorted(net_kw.items())),
               tuple(np.asarray(k).tobytes() for k in klist))
        cache = simulation_cell.__dict__.setdefault('_ds_cache', {})
        if key not in cache:
            tables = cache.get('tables')
            if tables is None:
                tables = cache['tables'] = EwaldTables(simulation_cell)
            cache[key] = cls(simulation_cell, klist, net_kw, tables, dtype)
        return cache[key]

    @classmethod
    def for_ewald(cls, simulation_cell, tables=None, dtype=torch.float64):
        """Ewald-only handle: a dummy minimal network description."""
        from .ewaldsum import EwaldTables
        from .supercell import make_klist
        cache = simulation_cell.__dict__.setdefault('_ds_cache', {})
        key = ('ewald', dtype)
        if key not in cache:
            tables = tables or cache.get('tables') or EwaldTables(simulation_cell)
            cache['tables'] = tables
            nk = dict(envelope_type='isotropic', bias_orbitals=False, use_last_layer=False, full_det=False,
                      hidden_dims=((64, 16), (64, 16)), determinants=8, distance_type='nu')
            if getattr(simulation_cell, 'AV', None) is None:
                from .supercell import set_symmetry_lat
                set_symmetry_lat(simulation_cell)
            klist = make_klist(simulation_cell)
            cache[key] = cls(simulation_cell, klist, nk, tables, dtype)
        return cache[key]

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                self.lib.ds_system_destroy(self.handle)
        except Exception:
            pass

    # ------------------------------------------------------------------ buffers
    def _check_x(self, x):
        if not x.is_cuda:
            raise RuntimeError('walkers must be a tensor on the ROCm device (no CPU path)')
        if x.dtype != self.dtype:
            raise TypeError(f'walkers are {x.dtype}, system was built for {self.dtype}')
        if x.dim() != 2 or x.shape[1] != 3 * self.n:
            raise ValueError(f'walkers must be (B, {3 * self.n}), got {tuple(x.shape)}')
        return x.contiguous()

    def _workspace(self, size_fn, *args, max_bytes=None, whole=False):
        """The cached device workspace, grown to what `size_fn(handle, *args)` reports or to the cap `max_bytes` (the library then
        walks the batch in more passes) -> its first `need` bytes, or with `whole` all of it.  A cap holds even when an earlier,
        larger call left a bigger buffer behind: the library sizes its passes by what it is given."""
        need = int(getattr(self.lib, size_fn)(self.handle, *args))
        if need < 0:
            _lib.check(1, size_fn)
        if max_bytes is not None:
            need = min(need, int(max_bytes))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws if whole else self._ws[:need]

    def workspace(self, B, max_bytes=None):
        return self._workspace('ds_workspace_bytes', int(B), max_bytes=max_bytes, whole=max_bytes is None)

    def pack_params(self, params):
        """Reference parameter tree (network.py:135-186) -> the flat device buffer of
        include/deepsolid_hip.h (`ds_param_layout`).  Cached on the leaves' versions."""
        return self.param_map.pack(params, self.device, self.dtype)

    # ------------------------------------------------------------------ calls
    def ewald(self, x):
        x = self._check_x(x)
        out = torch.empty(x.shape[0], 3, dtype=self.dtype, device=self.device)
        if x.shape[0] == 0:
            return out
        _lib.check(self.lib.ds_ewald(self.handle, _ptr(x), x.shape[0], _ptr(out), _stream()), 'ds_ewald')
        return out

    def local_energy(self, params, x, want_logpsi=False, ws_bytes=None):
        x = self._check_x(x)
        B = x.shape[0]
        p = self.pack_params(params)
        ws = self.workspace(B, ws_bytes)
        ke = torch.empty(B, 2, dtype=self.dtype, device=self.device)
        ew = torch.empty(B, dtype=self.dtype, device=self.device)
        la = torch.empty(B, dtype=self.dtype, device=self.device) if want_logpsi else None
        ph = torch.empty(B, 2, dtype=self.dtype, device=self.device) if want_logpsi else None
        if B == 0:
            return ke, ew, la, ph
        _lib.check(self.lib.ds_local_energy(self.handle, _ptr(p), _ptr(x), B, _ptr(ke), _ptr(ew), _ptr(la), _ptr(ph),
                                            _ptr(ws), ws.numel(), _stream()), 'ds_local_energy')
        return ke, ew, la, ph

    def logpsi(self, params, x, ws_bytes=None):
        x = self._check_x(x)
        B = x.shape[0]
        p = self.pack_params(params)
        ws = self.workspace(B, ws_bytes)
        la = torch.empty(B, dtype=self.dtype, device=self.device)
        ph = torch.empty(B, 2, dtype=self.dtype, device=self.device)
        if B == 0:
            return la, ph
        _lib.check(self.lib.ds_logpsi(self.handle, _ptr(p), _ptr(x), B, _ptr(la), _ptr(ph), _ptr(ws), ws.numel(),
                                      _stream()), 'ds_logpsi')
        return la, ph

    def logpsi_grad(self, params, x, ws_bytes=None):
        """-> (log|psi| (B,), grad (B, 3N) complex: Re = grad log|psi|, Im = grad arg psi).  `ws_bytes` caps the workspace: the
        library then walks the batch in chunks, as `logpsi` and `local_energy` do."""
        x = self._check_x(x)
        B = x.shape[0]
        p = self.pack_params(params)
        ws = self.workspace(B, ws_bytes)
        la = torch.empty(B, dtype=self.dtype, device=self.device)
        gr = torch.empty(B, 3 * self.n, 2, dtype=self.dtype, device=self.device)
        if B:
            _lib.check(self.lib.ds_logpsi_grad(self.handle, _ptr(p), _ptr(x), B, _ptr(la), _ptr(None), _ptr(gr), _ptr(ws),
                                               ws.numel(), _stream()), 'ds_logpsi_grad')
        return la, torch.view_as_complex(gr)

    def logpsi_vjp(self, params, x, cot, max_bytes=None):
        """Packed parameter gradient of sum_b Re(conj(cot_b) * log psi_b), log psi = log|psi| + i arg psi
        (`ds_logpsi_vjp`): cot (B,) complex or (B, 2) real.  -> (flat grad (param_count,), log|psi| (B,),
        phase (B,) complex).  `unpack_grad` turns the flat vector into the reference's parameter tree."""
        x = self._check_x(x)
        B = x.shape[0]
        if cot.is_complex():
            cot = torch.view_as_real(cot)
        cot = cot.to(device=self.device, dtype=self.dtype).contiguous()
        if tuple(cot.shape) != (B, 2):
            raise ValueError(f'cot must be ({B},) complex or ({B}, 2), got {tuple(cot.shape)}')
        p = self.pack_params(params)
        if B == 0:
            return (torch.zeros(self.param_count, dtype=self.dtype, device=self.device),
                    torch.empty(0, dtype=self.dtype, device=self.device),
                    torch.empty(0, dtype=torch.complex128 if self.dtype == torch.float64 else torch.complex64, device=self.device))
        ws = self._workspace('ds_vjp_workspace_bytes', int(B), max_bytes=max_bytes)
        grad = torch.empty(self.param_count, dtype=self.dtype, device=self.device)
        la = torch.empty(B, dtype=self.dtype, device=self.device)
        ph = torch.empty(B, 2, dtype=self.dtype, device=self.device)
        _lib.check(self.lib.ds_logpsi_vjp(self.handle, _ptr(p), _ptr(x), B, _ptr(cot), _ptr(grad), _ptr(la), _ptr(ph), _ptr(ws),
                                          ws.numel(), _stream()), 'ds_logpsi_vjp')
        return grad, la, torch.view_as_complex(ph)

    def logpsi_jacobian(self, params, x, out=None, max_bytes=None):
        """Per-walker Jacobian of log psi = log|psi| + i arg psi in the packed parameters (`ds_logpsi_jacobian`):
        -> (J (2B, param_count): row b = d log|psi_b| / d theta, row B + b = d arg psi_b / d theta; log|psi| (B,); phase (B,)
        complex).  `out`: a (2B, ld) tensor of the system's dtype with unit column stride and ld >= param_count to write into (J is
        then its first param_count columns; the others are not touched).  `max_bytes` caps the workspace: the library then walks
        the batch in more chunks, with the same bits."""
        x = self._check_x(x)
        B = x.shape[0]
        p = self.pack_params(params)
        P = self.param_count
        if out is None:
            out = torch.empty(2 * B, P, dtype=self.dtype, device=self.device)
        if (out.dtype != self.dtype or not out.is_cuda or out.dim() != 2 or out.shape[0] != 2 * B or out.shape[1] < P
                or (B > 0 and (out.stride(1) != 1 or out.stride(0) < out.shape[1]))):
            raise ValueError(f'out must be a ({2 * B}, >= {P}) {self.dtype} device tensor with contiguous rows')
        la = torch.empty(B, dtype=self.dtype, device=self.device)
        ph = torch.empty(B, 2, dtype=self.dtype, device=self.device)
        if B > 0:
            ws = self._workspace('ds_jacobian_workspace_bytes', int(B), max_bytes=max_bytes)
            _lib.check(self.lib.ds_logpsi_jacobian(self.handle, _ptr(p), _ptr(x), B, _ptr(out), int(out.stride(0)), _ptr(la), _ptr(ph),
                                                   _ptr(ws), ws.numel(), _stream()), 'ds_logpsi_jacobian')
        return out[:, :P], la, torch.view_as_complex(ph)

    # Linear algebra on a Jacobian (`ds_minsr_*`): no system handle, any (R, P).  jac: (R, >= P) float64 / float32 device tensor
    # with contiguous rows, of which the first P columns count; vectors and G are float64.
    @staticmethod
    def _minsr_jac(jac, P=None):
        if not jac.is_cuda or jac.dim() != 2 or jac.dtype not in _DTYPES or jac.stride(1) != 1:
            raise ValueError('jac must be a 2-d float64 / float32 device tensor with contiguous rows')
        P = jac.shape[1] if P is None else int(P)
        if not 0 < P <= jac.shape[1] or jac.shape[0] < 1:
            raise ValueError(f'jac is {tuple(jac.shape)}: P = {P} columns do not fit')
        return _lib.load(), int(jac.shape[0]), P, int(jac.stride(0))

    @staticmethod
    def _minsr_ws(lib, device, fn, *args):
        need = int(getattr(lib, fn)(*args))
        if need < 0:
            _lib.check(1, fn)
        return torch.empty(max(need, 8), dtype=torch.uint8, device=device)

    @staticmethod
    def minsr_gram(jac, P=None):
        """G = J J^T (R, R) float64, exactly symmetric (`ds_minsr_gram`)."""
        lib, R, P, ld = DeviceSystem._minsr_jac(jac, P)
        ws = DeviceSystem._minsr_ws(lib, jac.device, 'ds_minsr_gram_workspace_bytes', R, P)
        G = torch.empty(R, R, dtype=torch.float64, device=jac.device)
        _lib.check(lib.ds_minsr_gram(_DTYPES[jac.dtype], _ptr(jac), R, P, ld, _ptr(G), _ptr(ws), ws.numel(), _stream()), 'ds_minsr_gram')
        return G

    @staticmethod
    def minsr_matvec(jac, v, transpose=False, P=None):
        """J v (R,) or, with `transpose`, J^T v (P,), float64 (`ds_minsr_matvec`)."""
        lib, R, P, ld = DeviceSystem._minsr_jac(jac, P)
        n_in, n_out = (R, P) if transpose else (P, R)
        v = v.to(device=jac.device, dtype=torch.float64).contiguous()
        if v.numel() != n_in:
            raise ValueError(f'v must hold {n_in} entries, got {v.numel()}')
        out = torch.empty(n_out, dtype=torch.float64, device=jac.device)
        _lib.check(lib.ds_minsr_matvec(_DTYPES[jac.dtype], 1 if transpose else 0, _ptr(jac), R, P, ld, _ptr(v), _ptr(out), _ptr(None), 0,
                                       _stream()), 'ds_minsr_matvec')
        return out

    @staticmethod
    def minsr_solve(G, rhs, scale=1.0, damping=1e-3, block=0):
        """zeta of (scale H G H + damping I) zeta = rhs in float64; H centres each consecutive `block` rows and columns
        (0: no centring) (`ds_minsr_solve`)."""
        if not G.is_cuda or G.dim() != 2 or G.shape[0] != G.shape[1] or G.dtype != torch.float64:
            raise ValueError('G must be a square float64 device tensor')
        lib, R = _lib.load(), int(G.shape[0])
        G = G.contiguous()
        rhs = rhs.to(device=G.device, dtype=torch.float64).contiguous()
        if rhs.numel() != R:
            raise ValueError(f'rhs must hold {R} entries, got {rhs.numel()}')
        need = int(lib.ds_minsr_solve_workspace_bytes(R, int(block)))
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device=G.device)       # (a refused shape: the call below names the reason)
        zeta = torch.empty(R, dtype=torch.float64, device=G.device)
        _lib.check(lib.ds_minsr_solve(R, int(block), float(scale), float(damping), _ptr(G), _ptr(rhs), _ptr(zeta), _ptr(ws), ws.numel(),
                                      _stream()), 'ds_minsr_solve')
        return zeta

    def pretrain_loss_vjp(self, params, x, targets, max_bytes=None):
        """Orbital-matching loss of pretrain.py:70-94 and its packed parameter gradient (`ds_pretrain_loss_vjp`).
        `targets`: the reference's list, one complex (B, n_s, n_s) tensor [walker, electron, orbital] per spin with
        electrons (what `hf.SCF.eval_orb_mat` returns, empty spins dropped); real (B, n_s, n_s, 2) is taken as well.  With
        `full_det` the block-diagonal target is formed inside the kernel.  The means run over THIS call's walkers.
        -> (loss: 0-d float64 device tensor, flat grad (param_count,)); `unpack_grad` gives the parameter tree."""
        x = self._check_x(x)
        B = x.shape[0]
        sizes = [n for n in self.nelec if n > 0]        # (a spin-down-only cell runs mirrored: its one target is `up` here)
        targets = list(targets)
        if len(targets) != len(sizes):
            raise ValueError(f'targets must hold one matrix per spin with electrons ({len(sizes)}), got {len(targets)}')
        tg = []
        for t, n in zip(targets, sizes):
            if not isinstance(t, torch.Tensor):
                t = torch.as_tensor(np.asarray(t))
            if t.is_complex():
                t = torch.view_as_real(t.resolve_conj())
            if tuple(t.shape) != (B, n, n, 2):
                raise ValueError(f'target must be ({B}, {n}, {n}) complex, got {tuple(t.shape)}')
            tg.append(t.to(device=self.device, dtype=self.dtype).contiguous())
        p = self.pack_params(params)
        if B == 0:
            return (torch.zeros((), dtype=torch.float64, device=self.device),
                    torch.zeros(self.param_count, dtype=self.dtype, device=self.device))
        ws = self._workspace('ds_pretrain_workspace_bytes', int(B), max_bytes=max_bytes)
        loss = torch.empty(1, dtype=torch.float64, device=self.device)
        grad = torch.empty(self.param_count, dtype=self.dtype, device=self.device)
        _lib.check(self.lib.ds_pretrain_loss_vjp(self.handle, _ptr(p), _ptr(x), B, _ptr(tg[0]), _ptr(tg[1] if len(tg) > 1 else None),
                                                 _ptr(loss), _ptr(grad), _ptr(ws), ws.numel(), _stream()), 'ds_pretrain_loss_vjp')
        return loss[0], grad

    def kfac_layout(self):
        """The KFAC blocks of the network (`ds_kfac_layout`): one dict per `repeated_dense` layer of the reference, in the
        order single[0..], double[0..], orbital[0..], with the keys kind ('single' | 'double' | 'orbital'), index,
        param_blocks (indices into `self.blocks`), has_bias, d_in (bias row included), d_out, repeats, a_offset, g_offset."""
        n = int(self.lib.ds_kfac_block_count(self.handle))
        if n < 0:
            _lib.check(1, 'ds_kfac_block_count')
        raw = (_lib.KfacBlock * n)()
        if int(self.lib.ds_kfac_layout(self.handle, raw, n)) != n:
            _lib.check(1, 'ds_kfac_layout')
        kinds = ('single', 'double', 'orbital')
        return [dict(kind=kinds[b.kind], index=int(b.index), param_blocks=[int(v) for v in b.param_blocks[:b.n_param_blocks]],
                     has_bias=bool(b.has_bias), d_in=int(b.d_in), d_out=int(b.d_out), repeats=int(b.repeats),
                     a_offset=int(b.a_offset), g_offset=int(b.g_offset)) for b in raw]

    def kfac_factors(self, params, x, want_grad=True, max_bytes=None, flat=False):
        """Kronecker factors of every tagged layer at walkers x (`ds_kfac_factors`): one value chain and one reverse sweep with
        the seed sqrt2 on every walker.  -> (factors: [(A (d_in, d_in), G (d_out, d_out))] views in the order of `kfac_layout`,
        already divided by B * repeats; grad_seed: packed gradient of sum_b sqrt2 log|psi_b|, or None without `want_grad`).
        `max_bytes` caps the workspace (the library then walks the batch in chunks).  `flat=True`: the flat factor buffer itself
        (the layout of `kfac_layout`: what `kfac_inverses` reads) in place of the list of views."""
        flat_out = bool(flat)
        if self.net_kw.get('envelope_type') == 'full':
            raise NotImplementedError("KFAC with envelope_type='full' is not supported: the reference tags its sigma as a "
                                      "curvature block of its own (qmc1, network.py:358-362), which has no factor kernel here")
        x = self._check_x(x)
        B = x.shape[0]
        p = self.pack_params(params)
        layout = self.kfac_layout()
        total = layout[-1]['g_offset'] + layout[-1]['d_out'] ** 2
        ws = self._workspace('ds_kfac_workspace_bytes', int(B), max_bytes=max_bytes)
        flat = torch.empty(total, dtype=self.dtype, device=self.device)
        grad = torch.empty(self.param_count, dtype=self.dtype, device=self.device) if want_grad else None
        _lib.check(self.lib.ds_kfac_factors(self.handle, _ptr(p), _ptr(x), B, _ptr(flat), _ptr(grad), _ptr(ws), ws.numel(),
                                            _stream()), 'ds_kfac_factors')
        if flat_out:
            return flat, grad
        return self.kfac_views(flat, layout), grad

    def kfac_views(self, flat, layout=None):
        """[(A, G)] views of a flat factor (or inverse) buffer, in the order of `kfac_layout`."""
        layout = layout or self.kfac_layout()
        return [(flat[b['a_offset']:b['a_offset'] + b['d_in'] ** 2].view(b['d_in'], b['d_in']),
                 flat[b['g_offset']:b['g_offset'] + b['d_out'] ** 2].view(b['d_out'], b['d_out'])) for b in layout]

    def kfac_inverses(self, factors_flat, ema_weight, damping):
        """Damped inverses of every block's factors (`ds_kfac_inverses`, reference utils.py:155-218): `factors_flat` holds the raw
        moving-average arrays in the flat layout of `kfac_factors(flat=True)`, their value is array / `ema_weight`; `damping` is
        l2_reg + damping.  -> the inverses in the same flat layout (`kfac_views` cuts it up), exactly symmetric."""
        layout = self.kfac_layout()
        total = layout[-1]['g_offset'] + layout[-1]['d_out'] ** 2
        f = factors_flat.to(device=self.device, dtype=self.dtype).contiguous()
        if f.numel() != total:
            raise ValueError(f'factors must hold {total} elements, got {f.numel()}')
        ws = self._workspace('ds_kfac_step_workspace_bytes')
        out = torch.empty(total, dtype=self.dtype, device=self.device)
        _lib.check(self.lib.ds_kfac_inverses(self.handle, _ptr(f), float(ema_weight), float(damping), _ptr(out), _ptr(ws), ws.numel(),
                                             _stream()), 'ds_kfac_inverses')
        return out

    def kfac_precondition(self, inverses_flat, v_flat):
        """`ds_kfac_precondition`: v_flat holds one row-major d_in x d_out matrix per block in layout order (`kfac_index` maps the
        packed gradient onto it).  -> (out_flat with out_b = A^-_b v_b G^-_b / R_b, sq_norm (n_blocks,) float64 = <out_b, v_b>)."""
        layout = self.kfac_layout()
        total = layout[-1]['g_offset'] + layout[-1]['d_out'] ** 2
        nv = sum(b['d_in'] * b['d_out'] for b in layout)
        inv = inverses_flat.to(device=self.device, dtype=self.dtype).contiguous()
        v = v_flat.to(device=self.device, dtype=self.dtype).contiguous()
        if inv.numel() != total or v.numel() != nv:
            raise ValueError(f'inverses / v must hold {total} / {nv} elements, got {inv.numel()} / {v.numel()}')
        ws = self._workspace('ds_kfac_step_workspace_bytes')
        out = torch.empty(nv, dtype=self.dtype, device=self.device)
        sq = torch.empty(len(layout), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.ds_kfac_precondition(self.handle, _ptr(inv), _ptr(v), _ptr(out), _ptr(sq), _ptr(ws), ws.numel(), _stream()),
                   'ds_kfac_precondition')
        return out, sq

    def kfac_index(self, params):
        """Index maps of the KFAC step for a parameter tree of this shape, built once (`ParamMap.kfac_index`)."""
        return self.param_map.kfac_index(self.kfac_layout(), params, self.device)

    def unpack_grad(self, flat, params):
        """Packed gradient -> a tree shaped like `params` (reference layout, network.py:135-186)."""
        return self.param_map.unpack(flat, params)

    def orbitals(self, params, x):
        x = self._check_x(x)
        B = x.shape[0]
        p = self.pack_params(params)
        ws = self.workspace(B)
        if self.net_kw.get('full_det', False):
            sizes = [self.n, 0]
        else:
            sizes = list(self.nelec)
        outs = [torch.empty(B, self.n_det, ns, ns, 2, dtype=self.dtype, device=self.device) if ns else None for ns in sizes]
        if B == 0:
            return [torch.view_as_complex(o) for o in outs if o is not None]
        _lib.check(self.lib.ds_orbitals(self.handle, _ptr(p), _ptr(x), B, _ptr(outs[0]), _ptr(outs[1]), _ptr(ws),
                                        ws.numel(), _stream()), 'ds_orbitals')
        return [torch.view_as_complex(o) for o in outs if o is not None]

    def mh_propose(self, x1, normal, width):
        x1 = self._check_x(x1)
        normal = self._check_x(normal)
        x2 = torch.empty_like(x1)
        _lib.check(self.lib.ds_mh_propose(self.handle, _ptr(x1), _ptr(normal), float(width), x1.shape[0], _ptr(x2),
                                          _stream()), 'ds_mh_propose')
        return x2

    def mh_accept(self, x1, lp1, x2, lp2, uniform, n_accept):
        """In-place select on x1 / lp1; n_accept (1,) is incremented."""
        _lib.check(self.lib.ds_mh_accept(self.handle, _ptr(x1), _ptr(lp1), _ptr(x2), _ptr(lp2), _ptr(uniform),
                                         x1.shape[0], _ptr(n_accept), _stream()), 'ds_mh_accept')

    def mh_propose_ex(self, mode, x1, normal, width, aux, scratch=None):
        """`ds_mh_propose_ex`: mode 1 asymmetric (aux = nuclei (A,3)), mode 2 drift (aux = grad log|psi| (B,3N))."""
        x1 = self._check_x(x1)
        normal = self._check_x(normal)
        aux = aux.to(device=self.device, dtype=self.dtype).contiguous()
        x2 = torch.empty_like(x1)
        n_aux = aux.shape[0] if mode == 1 else 0
        _lib.check(self.lib.ds_mh_propose_ex(self.handle, int(mode), _ptr(x1), _ptr(normal), float(width), _ptr(aux), int(n_aux),
                                             x1.shape[0], _ptr(x2), _ptr(scratch), _stream()), 'ds_mh_propose_ex')
        return x2

    def mh_accept_ex(self, mode, x1, lp1, x2, logabs2, uniform, normal, width, aux1, aux2, n_accept, scratch=None):
        """`ds_mh_accept_ex`: in-place select on x1 / lp1; n_accept (1,) is incremented."""
        cv = lambda t: None if t is None else t.to(device=self.device, dtype=self.dtype).contiguous()
        aux1, aux2, normal = cv(aux1), cv(aux2), cv(normal)
        n_aux = aux1.shape[0] if mode == 1 else 0
        _lib.check(self.lib.ds_mh_accept_ex(self.handle, int(mode), _ptr(x1), _ptr(lp1), _ptr(x2), _ptr(cv(logabs2)), _ptr(cv(uniform)),
                                            _ptr(normal), float(width), _ptr(aux1), _ptr(aux2), int(n_aux), x1.shape[0],
                                            _ptr(n_accept), _ptr(scratch), _stream()), 'ds_mh_accept_ex')

    def mcmc_step(self, params, x, lp, steps, width, seed=0, offset=0, normals=None, uniforms=None, lp_valid=False,
                  n_accept=None, first_electron=None, importance=False, atoms=None):
        """`ds_mcmc_step`: `steps` all-electron Metropolis moves on x (B,3N) / lp (B,) IN PLACE, enqueued without a host
        synchronisation.  Noise from the in-kernel Philox stream (seed, offset) or replayed from `normals`
        (steps,B,3N) / `uniforms` (steps,B).  -> n_accept (1,) device tensor (incremented).
        `first_electron` = e: `ds_mcmc_step_one_electron` instead -- move i displaces electron (e + i) % N only
        (explicit normals are then (steps,B,3)).  `importance=True`: `ds_mcmc_step_importance`, the drift-biased move.
        `atoms` (A,3): `ds_mcmc_step_asymmetric`, step widths scaled by the harmonic mean of the nuclear distances."""
        x = self._check_x(x)
        B = x.shape[0]
        p = self.pack_params(params)
        if n_accept is None:
            n_accept = torch.zeros(1, dtype=self.dtype, device=self.device)
        if B == 0 or steps == 0 and lp_valid:
            return n_accept
        if normals is not None:
            normals = normals.to(device=self.device, dtype=self.dtype).contiguous()
            uniforms = uniforms.to(device=self.device, dtype=self.dtype).contiguous()
            width3 = 3 * self.n if first_electron is None else 3
            if tuple(normals.shape) != (steps, B, width3) or tuple(uniforms.shape) != (steps, B):
                raise ValueError('explicit noise must be normals (steps, B, 3N) -- (steps, B, 3) for one-electron moves -- '
                                 'and uniforms (steps, B)')
        ws = self._workspace('ds_mcmc_workspace_bytes', int(B), whole=True)
        if atoms is not None:
            atoms = torch.as_tensor(atoms, dtype=self.dtype, device=self.device).reshape(-1, 3).contiguous()
            _lib.check(self.lib.ds_mcmc_step_asymmetric(
                self.handle, _ptr(p), _ptr(x), _ptr(lp), B, int(steps), float(width), _ptr(atoms), int(atoms.shape[0]),
                int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), _ptr(normals), _ptr(uniforms), int(bool(lp_valid)),
                _ptr(n_accept), _ptr(ws), ws.numel(), _stream()), 'ds_mcmc_step_asymmetric')
            return n_accept
        if importance:
            _lib.check(self.lib.ds_mcmc_step_importance(
                self.handle, _ptr(p), _ptr(x), _ptr(lp), B, int(steps), float(width), int(seed) & (2 ** 64 - 1),
                int(offset) & (2 ** 64 - 1), _ptr(normals), _ptr(uniforms), int(bool(lp_valid)), _ptr(n_accept), _ptr(ws),
                ws.numel(), _stream()), 'ds_mcmc_step_importance')
            return n_accept
        if first_electron is not None:
            _lib.check(self.lib.ds_mcmc_step_one_electron(
                self.handle, _ptr(p), _ptr(x), _ptr(lp), B, int(steps), int(first_electron), float(width), int(seed) & (2 ** 64 - 1),
                int(offset) & (2 ** 64 - 1), _ptr(normals), _ptr(uniforms), int(bool(lp_valid)), _ptr(n_accept), _ptr(ws),
                ws.numel(), _stream()), 'ds_mcmc_step_one_electron')
            return n_accept
        _lib.check(self.lib.ds_mcmc_step(self.handle, _ptr(p), _ptr(x), _ptr(lp), B, int(steps), float(width),
                                         int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), _ptr(normals), _ptr(uniforms),
                                         int(bool(lp_valid)), _ptr(n_accept), _ptr(ws), ws.numel(), _stream()),
                   'ds_mcmc_step')
        return n_accept

    def one_body_ratios(self, params, x, n_samples, kvec=None, first_electron=0, seed=0, offset=0, shifts=None, nk_sums=None,
                        want_ratios=False, want_shifts=False, max_bytes=None):
        """`ds_one_body_ratios`: per walker `n_samples` ratios q = psi(R') / psi(R) with electron (first_electron + m) % N moved by a
        shift uniform in the simulation cell (in-kernel Philox stream (seed, offset); `shifts` (B, M, 3) replays given ones), folded
        into the momentum sums nk_sums[spin][k] += q exp(-i k.s) for the Cartesian points `kvec` (n_k, 3), n_k <= 512.
        `nk_sums`: float64 device tensor (2, n_k, 2) that is ADDED to (None: a fresh zero one).  `max_bytes` caps the workspace:
        the library then walks the samples in more chunks, with bit-identical results.
        -> dict(nk_sums (2, n_k, 2) or None without kvec, n_bad (2,) int64 device tensor: samples left out because q was not
        finite, ratios (B, M) complex with `want_ratios`, shifts (B, M, 3) with `want_shifts`).  No host synchronisation."""
        x = self._check_x(x)
        B, M = x.shape[0], int(n_samples)
        p = self.pack_params(params)
        kv = None
        n_k = 0
        if kvec is not None:
            kv = kvec if isinstance(kvec, torch.Tensor) else torch.as_tensor(np.asarray(kvec, dtype=np.float64))
            kv = kv.to(device=self.device, dtype=torch.float64).reshape(-1, 3).contiguous()
            n_k = int(kv.shape[0])
        if n_k:
            if nk_sums is None:
                nk_sums = torch.zeros(2, n_k, 2, dtype=torch.float64, device=self.device)
            elif not (nk_sums.is_cuda and nk_sums.dtype == torch.float64 and nk_sums.is_contiguous() and tuple(nk_sums.shape) == (2, n_k, 2)):
                raise ValueError(f'nk_sums must be a contiguous float64 device tensor of shape (2, {n_k}, 2)')
        else:
            kv = nk_sums = None
        if shifts is not None:
            shifts = shifts.to(device=self.device, dtype=self.dtype).contiguous()
            if tuple(shifts.shape) != (B, M, 3):
                raise ValueError(f'shifts must be ({B}, {M}, 3), got {tuple(shifts.shape)}')
        ratios = torch.empty(B, M, 2, dtype=self.dtype, device=self.device) if want_ratios else None
        out_s = torch.empty(B, M, 3, dtype=self.dtype, device=self.device) if want_shifts else None
        n_bad = torch.zeros(2, dtype=torch.int64, device=self.device)
        ws = self._workspace('ds_one_body_workspace_bytes', int(B), M, max_bytes=max_bytes) if B >= 1 and M >= 1 else \
            self.workspace(max(B, 1))                  # (the library refuses B < 1 / n_samples < 1 itself)
        _lib.check(self.lib.ds_one_body_ratios(self.handle, _ptr(p), _ptr(x), B, M, int(first_electron), int(seed) & (2 ** 64 - 1),
                                               int(offset) & (2 ** 64 - 1), _ptr(shifts), _ptr(kv), n_k, _ptr(nk_sums), _ptr(ratios),
                                               _ptr(out_s), _ptr(n_bad), _ptr(ws), ws.numel(), _stream()), 'ds_one_body_ratios')
        return dict(nk_sums=nk_sums, n_bad=n_bad, ratios=torch.view_as_complex(ratios) if want_ratios else None, shifts=out_s)

    def spin_exchange_ratios(self, params, x, n_pairs=None, first_pair=0, sums=None, want_ratios=False, want_walker=False,
                             max_bytes=None):
        """`ds_spin_exchange_ratios`: per walker `n_pairs` ratios q = psi(P_p R) / psi(R), P_p exchanging the positions of the up
        electron i and the down electron j of pair p = i n_dn + (j - n_up); sample m takes pair (first_pair + m) % P, P = n_up n_dn
        (default n_pairs: P, every pair once).  No random numbers.  `sums`: float64 device tensor (4,) that is ADDED to (None: a
        fresh zero one) = [sum_w Re t_w, sum_w Im t_w, sum_w (Re t_w)^2, good walkers] with t_w = sum_m q_{w,m}; a walker with a
        non-finite q is left out and counted.  `max_bytes` caps the workspace: more chunks, bit-identical results.
        -> dict(sums (4,), n_bad (1,) int64 device tensor, ratios (B, M) complex with `want_ratios`, walker (B,) complex128 with
        `want_walker`: NaN for a bad walker).  <S^2> = S_z (S_z + 1) + n_dn - (P / M) sums[0] / sums[3] (`estimator.SpinSquared`).
        No host synchronisation."""
        x = self._check_x(x)
        B = x.shape[0]
        M = self.nelec[0] * self.nelec[1] if n_pairs is None else int(n_pairs)
        p = self.pack_params(params)
        if sums is None:
            sums = torch.zeros(4, dtype=torch.float64, device=self.device)
        elif not (sums.is_cuda and sums.dtype == torch.float64 and sums.is_contiguous() and tuple(sums.shape) == (4,)):
            raise ValueError('sums must be a contiguous float64 device tensor of shape (4,)')
        ratios = torch.empty(B, M, 2, dtype=self.dtype, device=self.device) if want_ratios and M >= 1 else None
        walker = torch.empty(B, 2, dtype=torch.float64, device=self.device) if want_walker else None
        n_bad = torch.zeros(1, dtype=torch.int64, device=self.device)
        ws = self._workspace('ds_spin_exchange_workspace_bytes', int(B), M, max_bytes=max_bytes) if B >= 1 and M >= 1 else \
            self.workspace(max(B, 1))                  # (the library refuses B < 1 / n_pairs < 1 itself)
        _lib.check(self.lib.ds_spin_exchange_ratios(self.handle, _ptr(p), _ptr(x), B, M, int(first_pair), _ptr(sums), _ptr(ratios),
                                                    _ptr(walker), _ptr(n_bad), _ptr(ws), ws.numel(), _stream()),
                   'ds_spin_exchange_ratios')
        return dict(sums=sums, n_bad=n_bad, ratios=torch.view_as_complex(ratios) if ratios is not None else None,
                    walker=torch.view_as_complex(walker) if want_walker else None)

    def force_cutoff(self, cutoff=None):
        """The cutoff r_c of the zero-variance force term (`estimator.force_cutoff` on the simulation cell): `cutoff`, or by default
        the Wigner-Seitz radius, which is also the largest value accepted (the same check the library makes)."""
        from .estimator import force_cutoff
        return force_cutoff(self.cell.a, cutoff)

    def ion_forces(self, x, drift=None, cutoff=None, sums=None, want_walker=True, max_bytes=None):
        """`ds_ion_forces` (csrc/ds_force.h): per walker and ion of the simulation cell the Hellmann-Feynman
        force of the Ewald energy, hf = -d(E_ei + E_ii)/dR_a, and with `drift` (B, 3N) = Re grad log psi (`logpsi_grad(...)[1].real`)
        the zero-variance force zv = hf + dF of Assaraf and Caffarel with the cutoff `cutoff` (default and maximum: the Wigner-Seitz
        radius).  NOT the full force: the Pulay term is missing, so hf and zv are exact only for an exact psi (bias first order in
        the error of psi; `logpsi_ion_vjp` gives d log psi / dR_a for the atoms of the primitive cell and `estimator.PrimitiveForces`
        the total force); all-electron ions only.  `sums`: float64 device tensor (12 A + 1,) that is ADDED to = per (a, c)
        [sum hf, sum hf^2, sum zv, sum zv^2] over the good walkers, then their number; it needs the drift.  A walker with a
        non-finite coordinate, drift or result is NaN, left out and counted.  `max_bytes` caps the workspace of `sums`: more
        passes, bit-identical results.  The ion-ion force is computed once on the host and cached on the system.
        -> dict(hf (B, A, 3) float64 or None without `want_walker`, zv likewise or None without a drift, n_bad (1,) int64 device
        tensor, sums).  No host synchronisation."""
        x = self._check_x(x)
        B = x.shape[0]
        A = int(self.tables.atom_coords.shape[0])
        r_c = self.force_cutoff(cutoff)
        if drift is not None:
            if not (drift.is_cuda and drift.dtype == self.dtype and tuple(drift.shape) == tuple(x.shape)):
                raise ValueError(f'drift must be a {self.dtype} device tensor of shape {tuple(x.shape)}')
            drift = drift.contiguous()
        if sums is not None:
            if not (sums.is_cuda and sums.dtype == torch.float64 and sums.is_contiguous() and tuple(sums.shape) == (12 * A + 1,)):
                raise ValueError(f'sums must be a contiguous float64 device tensor of shape ({12 * A + 1},)')
            if drift is None:
                raise ValueError('sums hold the zero-variance force too: they need the drift')
        if not want_walker and sums is None:
            raise ValueError('nothing to compute: neither the walker forces nor sums are asked for')
        hf = torch.empty(B, A, 3, dtype=torch.float64, device=self.device) if want_walker else None
        zv = torch.empty(B, A, 3, dtype=torch.float64, device=self.device) if want_walker and drift is not None else None
        n_bad = torch.zeros(1, dtype=torch.int64, device=self.device)
        if B == 0:
            return dict(hf=hf, zv=zv, n_bad=n_bad, sums=sums)
        if getattr(self, '_ion_ion_force', None) is None:
            from .ewaldsum import ion_ion_forces
            self._ion_ion_force = torch.as_tensor(ion_ion_forces(self.cell, tables=self.tables), dtype=torch.float64, device=self.device)
        ws = self._workspace('ds_ion_forces_workspace_bytes', int(B), max_bytes=max_bytes) if sums is not None else None
        _lib.check(self.lib.ds_ion_forces(self.handle, _ptr(x), _ptr(drift), B, r_c, _ptr(self._ion_ion_force), _ptr(hf), _ptr(zv),
                                          _ptr(sums), _ptr(n_bad), _ptr(ws), ws.numel() if ws is not None else 0, _stream()),
                   'ds_ion_forces')
        return dict(hf=hf, zv=zv, n_bad=n_bad, sums=sums)

    def stress(self, x, grad=None, sums=None, want_walker=True, max_bytes=None):
        """`ds_stress` (csrc/ds_stress.h): per walker the strain derivative dE / d eps of the energy, as
        symmetric tensors in the component order xx, yy, zz, yz, xz, xy, in Hartree: parts (B, 4, 6) float64 with the rows
        kin (-sum_i Re(d_i conj d_i^T), d = `grad` (B, 3N) complex = `logpsi_grad(...)[1]`; zero without `grad`), ee, ei (the Ewald sums
        of `ewald` under a homogeneous strain: alpha, the G list and the minimal images held fixed) and total = kin + ee + ei + the
        ion-ion constant.  The stress is total / volume, the pressure -tr / 3 of that (`estimator.StressTensor`).  NOT the full
        stress of a variational psi: the change of psi with the cell at fixed parameters is missing; all-electron ions only.
        `sums`: float64 device tensor (49,) that is ADDED to = per row and component [sum, sum of squares] over the good walkers, then
        their number; it needs `grad`.  A walker with a non-finite coordinate, gradient or result is NaN, left out and counted.
        `max_bytes` caps the workspace of `sums`: more passes, bit-identical results.  The ion-ion constant
        (`ewaldsum.ion_ion_stress`) is computed once on the host and cached on the system.
        -> dict(parts (B, 4, 6) or None without `want_walker`, n_bad (1,) int64 device tensor, sums).  No host synchronisation."""
        x = self._check_x(x)
        B = x.shape[0]
        if grad is not None:
            if not (grad.is_cuda and grad.is_complex() and torch.view_as_real(grad).dtype == self.dtype and
                    tuple(grad.shape) == tuple(x.shape)):
                raise ValueError(f'grad must be a complex device tensor of shape {tuple(x.shape)} with {self.dtype} parts')
            grad = torch.view_as_real(grad.contiguous())
        if sums is not None:
            if not (sums.is_cuda and sums.dtype == torch.float64 and sums.is_contiguous() and tuple(sums.shape) == (49,)):
                raise ValueError('sums must be a contiguous float64 device tensor of shape (49,)')
            if grad is None:
                raise ValueError('sums hold the kinetic rows too: they need grad')
        if not want_walker and sums is None:
            raise ValueError('nothing to compute: neither the walker tensors nor sums are asked for')
        parts = torch.empty(B, 4, 6, dtype=torch.float64, device=self.device) if want_walker else None
        n_bad = torch.zeros(1, dtype=torch.int64, device=self.device)
        if B == 0:
            return dict(parts=parts, n_bad=n_bad, sums=sums)
        if getattr(self, '_ion_ion_stress', None) is None:
            from .ewaldsum import VOIGT, ion_ion_stress
            ii = ion_ion_stress(self.cell, tables=self.tables)
            self._ion_ion_stress = torch.as_tensor(np.array([ii[a, b] for a, b in VOIGT]), dtype=torch.float64, device=self.device)
        ws = self._workspace('ds_stress_workspace_bytes', int(B), max_bytes=max_bytes) if sums is not None else None
        _lib.check(self.lib.ds_stress(self.handle, _ptr(x), _ptr(grad), B, _ptr(self._ion_ion_stress), _ptr(parts), _ptr(sums),
                                      _ptr(n_bad), _ptr(ws), ws.numel() if ws is not None else 0, _stream()), 'ds_stress')
        return dict(parts=parts, n_bad=n_bad, sums=sums)

    def logpsi_ion_vjp(self, params, x, cot, max_bytes=None):
        """`ds_logpsi_ion_vjp` (csrc/ds_iongrad.h): per walker the gradient of
        cot_b[0] log|psi_b| + cot_b[1] arg psi_b in the positions of the A atoms of the PRIMITIVE cell (`self.prim_atoms`), the
        only ions psi sees; moving atom a moves all its images of the simulation cell together.  cot (B,) complex or (B, 2) real,
        the convention of `logpsi_vjp`.  -> (out (B, A, 3) float64 for either dtype, NOT summed over the batch; log|psi| (B,);
        phase (B,) complex).  `max_bytes` caps the workspace: more passes, the same bits."""
        x = self._check_x(x)
        B = x.shape[0]
        if cot.is_complex():
            cot = torch.view_as_real(cot)
        cot = cot.to(device=self.device, dtype=self.dtype).contiguous()
        if tuple(cot.shape) != (B, 2):
            raise ValueError(f'cot must be ({B},) complex or ({B}, 2), got {tuple(cot.shape)}')
        p = self.pack_params(params)
        A = self.n_atoms_prim
        out = torch.empty(B, A, 3, dtype=torch.float64, device=self.device)
        la = torch.empty(B, dtype=self.dtype, device=self.device)
        ph = torch.empty(B, 2, dtype=self.dtype, device=self.device)
        if B > 0:
            ws = self._workspace('ds_ion_vjp_workspace_bytes', int(B), max_bytes=max_bytes)
            _lib.check(self.lib.ds_logpsi_ion_vjp(self.handle, _ptr(p), _ptr(x), B, _ptr(cot), _ptr(out), _ptr(la), _ptr(ph), _ptr(ws),
                                                  ws.numel(), _stream()), 'ds_logpsi_ion_vjp')
        return out, la, torch.view_as_complex(ph)

    def logpsi_ion_grad(self, params, x, max_bytes=None):
        """O = d log psi / d R_a per walker and atom of the primitive cell, complex (B, A, 3): Re = d log|psi|, Im = d arg psi, as
        `logpsi_grad` gives them in the walker coordinates.  Two `logpsi_ion_vjp` calls, cot = (1, 0) and (0, 1)."""
        B = x.shape[0]
        one = torch.zeros(B, 2, dtype=self.dtype, device=self.device)
        one[:, 0] = 1
        re = self.logpsi_ion_vjp(params, x, one, max_bytes=max_bytes)[0]
        im = self.logpsi_ion_vjp(params, x, one.flip(1), max_bytes=max_bytes)[0]
        return torch.complex(re, im)

    def dmc_state(self, x, weight=None, ecp=False):
        """Fresh DMC walker state for `dmc_step(..., state_valid=False)`: dict of the six caller-owned device buffers (x is copied;
        logabs, phase, drift and eloc are filled by the first call; weights are 1 or `weight`).  `ecp=True` adds the seventh, 'epp'
        (B, 3) float64 = (E_loc, Re E_nl, Im E_nl), which `dmc_step(..., ecp=...)` needs; the six others remain a valid state of the
        plain call."""
        x = self._check_x(x).clone()
        B = x.shape[0]
        f64 = dict(dtype=torch.float64, device=self.device)
        w = torch.ones(B, **f64) if weight is None else torch.as_tensor(weight).to(**f64).reshape(B).clone()
        state = dict(x=x, logabs=torch.zeros(B, dtype=self.dtype, device=self.device),
                     phase=torch.zeros(B, 2, dtype=self.dtype, device=self.device), drift=torch.zeros_like(x),
                     eloc=torch.zeros(B, **f64), weight=w)
        if ecp:
            state['epp'] = torch.zeros(B, 3, **f64)
        return state

    def _check_dmc_state(self, state, ecp=False):
        B = state['x'].shape[0]
        shapes = dict(x=((B, 3 * self.n), self.dtype), logabs=((B,), self.dtype), phase=((B, 2), self.dtype),
                      drift=((B, 3 * self.n), self.dtype), eloc=((B,), torch.float64), weight=((B,), torch.float64))
        if ecp or 'epp' in state:
            if 'epp' not in state:
                raise ValueError("DMC with a pseudopotential needs the state entry 'epp' (dmc_state(..., ecp=True))")
            shapes['epp'] = ((B, 3), torch.float64)
        for k, (shape, dt) in shapes.items():
            t = state[k]
            if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shape):
                raise ValueError(f'DMC state entry {k!r} must be a contiguous {dt} device tensor of shape {shape}')
        return B

    def dmc_step(self, params, state, steps, tau, tau_eff=None, e_trial=0.0, e_ref=0.0, e_cut=0.0, node_mode=0, branch_every=1,
                 seed=0, offset=0, normals=None, uniforms=None, comb_uniforms=None, state_valid=True, want_parents=False,
                 max_bytes=None, ecp=None, pair_capacity=None, rotations=None, want_pairs=False, tmoves=False, tmove_uniforms=None,
                 want_tmoves=False):
        """`ds_dmc_step`: `steps` fixed-phase DMC steps on the walker state IN PLACE (dict of x, logabs, phase, drift, eloc, weight:
        `dmc_state`), enqueued without a host synchronisation; the algorithm is stated in include/deepsolid_hip.h.  Noise from
        the in-kernel Philox stream (seed, offset) or replayed from `normals` (steps,B,3N), `uniforms` (steps,B) and
        `comb_uniforms` (steps,) float64 -- all three or none.  `max_bytes` caps the workspace: more chain chunks.
        -> dict(stats (steps, 9) float64 device tensor, parents (steps, B) int32 with `want_parents`).

        `ecp` (an `EcpTables` or a `pseudopotential.SemiLocalECP`, as in `ecp_energy`): `ds_dmc_step_ecp`, the locality
        approximation; the state then has the seventh array 'epp'.  That call SYNCHRONISES the stream once per step, and once more
        for an initialisation (the pair total of every pseudopotential evaluation).  `rotations` (steps + 1, B, 3, 3) float64
        goes with the explicit noise: all four or none.  `pair_capacity` defaults to the hard bound B * N * (atoms whose species
        has a non-local channel), which cannot overflow; where the pair records of that bound exceed `ECP_PAIR_BUDGET` bytes the
        default is B * N, and on overflow the call is repeated once with the number the library reports, continuing from the
        steps that were completed.  The dict gains ecp_stats (steps, 3) float64 = per step sum w E_loc, sum w Re E_nl, sum w Im E_nl,
        pairs (steps + 1,) int64 with `want_pairs` (entry 0: the initialisation), and pair_capacity.

        `tmoves=True` (with `ecp`): `ds_dmc_step_tmove`, Casula's T-moves.  The pseudopotential is evaluated after the decision, at
        the position the walker then has; 'eloc' is the chain part alone and 'epp' the triple of the walker's last evaluation.
        `tmove_uniforms` (steps, B) float64 joins the explicit noise (all five or none), `rotations` is (steps, B, 3, 3) and the
        initialisation evaluates no pseudopotential.  ecp_stats is (steps, 4): the fourth column counts the walkers that made a
        T-move; pairs is (steps,); the dict gains energy (steps, B) float64, the branching energy of every walker, and tmoves
        (steps, B) int32 with `want_tmoves`: the walker-local configuration pair * N_q + q of the move taken, or -1."""
        if tmoves and ecp is None:
            raise ValueError('tmoves=True needs a pseudopotential (ecp=...)')
        if (tmove_uniforms is not None or want_tmoves) and not tmoves:
            raise ValueError('tmove_uniforms and want_tmoves go with tmoves=True')
        if ecp is None and (rotations is not None or pair_capacity is not None or want_pairs):
            raise ValueError('rotations, pair_capacity and want_pairs go with a pseudopotential (ecp=...)')
        v = _DMC_VARIANTS['plain' if ecp is None else 'tmove' if tmoves else 'ecp']
        B = self._check_dmc_state(state, ecp=ecp is not None)
        steps, n, tmoves = int(steps), max(int(steps), 1), bool(tmoves)
        if ecp is not None:
            ecp = self._ecp_tables(ecp)
        p = self.pack_params(params)
        f64 = dict(dtype=torch.float64, device=self.device)
        # the explicit noise in the entry's order: all of it or none (the library refuses a part of it)
        noise = dict(normals=normals, uniforms=uniforms, comb_uniforms=comb_uniforms, rotations=rotations, tmove_uniforms=tmove_uniforms)
        noise = {k: noise[k] for k, _, _ in v.noise}
        explicit = all(t is not None for t in noise.values())
        if explicit:
            bad = []
            for k, is_f64, shape in v.noise:
                noise[k] = noise[k].to(device=self.device, dtype=torch.float64 if is_f64 else self.dtype).contiguous()
                if tuple(noise[k].shape) != (steps + (v.lead if k == 'rotations' else 0),) + shape(B, 3 * self.n):
                    bad.append(k)
            if bad:
                raise ValueError('tmove_uniforms must be (steps, B)' if bad == ['tmove_uniforms'] else v.noise_message)
        if ecp is None:
            cap = None
        elif pair_capacity is None:
            src = ecp.ecp
            n_nl = int(np.count_nonzero(np.asarray(src.n_l)[np.asarray(src.atom_species)] > 0))
            cap = B * self.n * max(n_nl, 1)
            if cap * (72 + 16 * ecp.n_quad) > self.ECP_PAIR_BUDGET:
                cap = B * self.n
        else:
            cap = int(pair_capacity)
        stats = torch.zeros(n, 9, **f64)
        parents = torch.empty(n, B, dtype=torch.int32, device=self.device) if want_parents else None
        ecp_stats = torch.zeros(n, v.columns, **f64) if ecp is not None else None
        pairs = torch.zeros(n + v.lead, dtype=torch.int64, device=self.device) if want_pairs else None
        choice = torch.full((n, B), -1, dtype=torch.int32, device=self.device) if want_tmoves else None
        energy = torch.zeros(n, B, **f64) if tmoves else None
        outs = [stats] + ([ecp_stats] if ecp is not None else []) + [parents] + ([pairs] if ecp is not None else []) + \
            ([choice, energy] if tmoves else [])
        keys = ('x', 'logabs', 'phase', 'drift', 'eloc', 'weight') + (('epp',) if ecp is not None else ())
        done, valid = 0, bool(state_valid)
        for attempt in range(2):                           # (a second time only after a pair capacity overflow)
            k, left = done, steps - done
            size_args = (int(B),) if ecp is None else (ecp.handle, int(B), cap)
            ws = self._workspace(v.ws_entry, *size_args, max_bytes=max_bytes) if 1 <= B <= 2 ** 20 and (ecp is None or cap >= 1) \
                else self.workspace(1)                     # (the library refuses such a B or capacity itself)
            n_done = C.c_int(0)
            cut = (lambda t: t[k:]) if explicit else (lambda t: t)
            rc = getattr(self.lib, v.entry)(
                self.handle, *((ecp.handle,) if ecp is not None else ()), _ptr(p), *[_ptr(state[key]) for key in keys], B, left, float(tau),
                float(tau if tau_eff is None else tau_eff), float(e_trial), float(e_ref), float(e_cut), int(node_mode), int(branch_every),
                int(seed) & (2 ** 64 - 1), (int(offset) + k) & (2 ** 64 - 1), *[_ptr(cut(t)) for t in noise.values()],
                *((cap,) if ecp is not None else ()), int(valid), *[_ptr(t[k:] if t is not None else None) for t in outs],
                *((C.byref(n_done),) if ecp is not None else ()), _ptr(ws), ws.numel(), _stream())
            if rc != 0 and attempt == 0 and ecp is not None and pair_capacity is None:
                m = re.search(r'pair capacity exceeded: the walkers have (\d+) pairs', self.lib.ds_last_error().decode())
                # (the comb's schedule counts the steps of a call: a continuation keeps it only from a multiple of branch_every)
                if m and (branch_every <= 1 or n_done.value % int(branch_every) == 0):
                    cap = int(m.group(1))
                    done += n_done.value
                    valid = valid or done > 0
                    continue
            _lib.check(rc, v.entry)
            break
        out = dict(stats=stats, parents=parents)
        if ecp is not None:
            out.update(ecp_stats=ecp_stats, pairs=pairs, pair_capacity=cap)
        if tmoves:
            out.update(tmoves=choice, energy=energy)
        return out

    ECP_PAIR_BUDGET = 1 << 30              # bytes of pair records up to which dmc_step's default capacity is the hard bound

    def _ecp_tables(self, ecp):
        if not isinstance(ecp, EcpTables):
            tables = ecp.__dict__.get('_ds_tables')
            if tables is None or tables.device != self.device:
                tables = ecp.__dict__['_ds_tables'] = EcpTables(ecp, device=self.device)
            ecp = tables
        return ecp

    def dmc_noise(self, B, steps, seed=0, offset=0):
        """`ds_dmc_noise`: what `dmc_step` draws in Philox mode for (seed, offset), as the arrays its explicit mode takes
        -> (normals (steps, B, 3N), uniforms (steps, B), comb_uniforms (steps,) float64)."""
        nz = torch.empty(steps, B, 3 * self.n, dtype=self.dtype, device=self.device)
        un = torch.empty(steps, B, dtype=self.dtype, device=self.device)
        xi = torch.empty(steps, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.ds_dmc_noise(0 if self.dtype == torch.float64 else 1, self.n, int(B), int(steps), int(seed) & (2 ** 64 - 1),
                                         int(offset) & (2 ** 64 - 1), _ptr(nz), _ptr(un), _ptr(xi), _stream()), 'ds_dmc_noise')
        return nz, un, xi

    def dmc_branch(self, state, xi, want_parents=True):
        """`ds_dmc_branch`: the fixed-population comb alone on a walker state, IN PLACE, with the given xi in [0, 1).  A state with
        the seventh array 'epp' has it gathered from the same parents.
        -> parents (B,) int32 device tensor (None without `want_parents`)."""
        B = self._check_dmc_state(state)
        want_parents, asked = want_parents or 'epp' in state, want_parents
        need = int(self.lib.ds_dmc_branch_workspace_bytes(0 if self.dtype == torch.float64 else 1, self.n, B))
        if need < 0:
            need = 256                                     # (the library refuses such a B itself)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        parents = torch.empty(B, dtype=torch.int32, device=self.device) if want_parents else None
        _lib.check(self.lib.ds_dmc_branch(0 if self.dtype == torch.float64 else 1, self.n, B, float(xi), _ptr(state['x']),
                                          _ptr(state['logabs']), _ptr(state['phase']), _ptr(state['drift']), _ptr(state['eloc']),
                                          _ptr(state['weight']), _ptr(parents), _ptr(self._ws), self._ws.numel(), _stream()),
                   'ds_dmc_branch')
        if 'epp' in state:
            state['epp'].copy_(state['epp'][parents.long()])        # (a skipped comb returns the identity)
        return parents if asked else None

    def ecp_energy(self, params, x, ecp, seed=0, offset=0, rotations=None, pair_capacity=None, want_pairs=False, want_ratios=False,
                   want_rotations=False, max_bytes=None):
        """`ds_ecp_energy`: the semi-local pseudopotential energy of every walker.  `ecp`: an `EcpTables` (or a
        `pseudopotential.SemiLocalECP`, whose device tables are then built once and kept on it).  One rotation of the quadrature
        points per walker and call from the in-kernel Philox stream (seed, offset) -- the caller advances `offset` by 1 per call --
        or `rotations` (B, 3, 3) float64 replays given ones.  `pair_capacity`: room for the (electron, ion) pairs inside the non-local
        cutoffs (default B * N, which always suffices when every atom's cutoff sphere holds each electron at most once); when the
        walkers have more the call is repeated once with the number the library reports.  `max_bytes` caps the workspace: more
        chunks, bit-identical results.
        -> dict(e_loc (B,) float64, e_nl (B,) complex128, pairs (B,) int64 with `want_pairs`, ratios (n_pairs * N_q,) complex with
        `want_ratios` (configuration pair * N_q + q, pairs ordered by (w, i, I)), rotations (B, 3, 3) with `want_rotations`,
        pair_capacity: the capacity the call ran with).
        The call synchronises the stream once (the pair total) and cannot be captured into a graph."""
        import re
        x = self._check_x(x)
        B = x.shape[0]
        ecp = self._ecp_tables(ecp)
        p = self.pack_params(params)
        if rotations is not None:
            rotations = rotations.to(device=self.device, dtype=torch.float64).contiguous()
            if tuple(rotations.shape) != (B, 3, 3):
                raise ValueError(f'rotations must be ({B}, 3, 3), got {tuple(rotations.shape)}')
        cap = B * self.n if pair_capacity is None else int(pair_capacity)
        energy = torch.empty(B, 3, dtype=torch.float64, device=self.device)
        pairs = torch.empty(B, dtype=torch.int64, device=self.device) if want_pairs or want_ratios else None
        rot = torch.empty(B, 3, 3, dtype=torch.float64, device=self.device) if want_rotations else None
        for attempt in range(2):
            ratios = torch.empty(max(cap, 1) * ecp.n_quad, 2, dtype=self.dtype, device=self.device) if want_ratios else None
            # (the library refuses B < 1 / pair_capacity < 1 / another cell itself, here already)
            ws = self._workspace('ds_ecp_workspace_bytes', ecp.handle, B, cap, max_bytes=max_bytes)
            rc = self.lib.ds_ecp_energy(self.handle, ecp.handle, _ptr(p), _ptr(x), B, int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1),
                                        _ptr(rotations), cap, _ptr(energy), _ptr(pairs), _ptr(ratios), _ptr(rot), _ptr(ws), ws.numel(),
                                        _stream())
            if rc != 0 and attempt == 0:
                m = re.search(r'pair capacity exceeded: the walkers have (\d+) pairs', self.lib.ds_last_error().decode())
                if m:
                    cap = int(m.group(1))
                    continue
            _lib.check(rc, 'ds_ecp_energy')
            break
        return dict(e_loc=energy[:, 0], e_nl=torch.complex(energy[:, 1], energy[:, 2]), pairs=pairs if want_pairs else None,
                    rotations=rot, pair_capacity=cap,
                    ratios=torch.view_as_complex(ratios)[:int(pairs.sum()) * ecp.n_quad] if want_ratios else None)

    def ecp_forces(self, params, x, ecp, seed=0, offset=0, rotations=None, pair_capacity=None, base=None, sums=None, want_walker=True,
                   max_bytes=None):
        """`ds_ecp_forces` (csrc/ds_ecp_force.h): per walker and ion of the simulation cell minus the derivative
        of the pseudopotential energy E_loc + E_nl of `ecp_energy` in the ion position, with psi held fixed as a function of the
        electron coordinates.  `ecp`, `seed`, `offset`, `rotations`, `pair_capacity` and the capacity retry are those of `ecp_energy`:
        the same (seed, offset) uses the same quadrature points.  `base` (B, A, 3) float64 is added per walker to form the total
        (meant for `ion_forces(x)['hf']`, the Ewald force with Z_eff).  `sums`: float64 device tensor (12 A + 1,) that is ADDED to
        = per (a, c) [sum pp, sum pp^2, sum tot, sum tot^2] over the good walkers, then their number; pp = loc + Re nl,
        tot = pp + base.  A walker with a non-finite coordinate, an electron exactly on a pseudo-ion or a non-finite result is NaN,
        left out and counted.  `max_bytes` caps the workspace: more chunks, bit-identical results.
        LIMITS: the Hellmann-Feynman part only (no Pulay term: the bias is first order in the error of psi); the delta term of the
        jump of a radial function at its cutoff is left out; one forward-Laplacian chain evaluation per quadrature configuration.
        -> dict(loc (B, A, 3) float64 and nl (B, A, 3) complex128, or None without `want_walker`; n_bad (1,) int64 device tensor;
        pairs (B,) int64; rotations (B, 3, 3) float64; pair_capacity: the capacity the call ran with; sums).
        The call synchronises the stream once (the pair total) and cannot be captured into a graph."""
        import re
        x = self._check_x(x)
        B = x.shape[0]
        ecp = self._ecp_tables(ecp)
        A = int(self.tables.atom_coords.shape[0])
        p = self.pack_params(params)
        if rotations is not None:
            rotations = rotations.to(device=self.device, dtype=torch.float64).contiguous()
            if tuple(rotations.shape) != (B, 3, 3):
                raise ValueError(f'rotations must be ({B}, 3, 3), got {tuple(rotations.shape)}')
        if base is not None:
            if not (base.is_cuda and base.dtype == torch.float64 and tuple(base.shape) == (B, A, 3)):
                raise ValueError(f'base must be a float64 device tensor of shape ({B}, {A}, 3)')
            base = base.contiguous()
        if sums is not None and not (sums.is_cuda and sums.dtype == torch.float64 and sums.is_contiguous()
                                     and tuple(sums.shape) == (12 * A + 1,)):
            raise ValueError(f'sums must be a contiguous float64 device tensor of shape ({12 * A + 1},)')
        if not want_walker and sums is None:
            raise ValueError('nothing to compute: neither the walker forces nor sums are asked for')
        cap = B * self.n if pair_capacity is None else int(pair_capacity)
        force = torch.empty(B, A, 3, 3, dtype=torch.float64, device=self.device) if want_walker else None
        pairs = torch.empty(B, dtype=torch.int64, device=self.device)
        rot = torch.empty(B, 3, 3, dtype=torch.float64, device=self.device)
        n_bad = torch.zeros(1, dtype=torch.int64, device=self.device)
        for attempt in range(2):
            # (the library refuses B < 1 / pair_capacity < 1 / another cell itself, here already)
            ws = self._workspace('ds_ecp_forces_workspace_bytes', ecp.handle, B, cap, max_bytes=max_bytes)
            rc = self.lib.ds_ecp_forces(self.handle, ecp.handle, _ptr(p), _ptr(x), B, int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1),
                                        _ptr(rotations), cap, _ptr(base), _ptr(force), _ptr(sums), _ptr(n_bad), _ptr(pairs), _ptr(rot),
                                        _ptr(ws), ws.numel(), _stream())
            if rc != 0 and attempt == 0:
                m = re.search(r'pair capacity exceeded: the walkers have (\d+) pairs', self.lib.ds_last_error().decode())
                if m:
                    cap = int(m.group(1))
                    continue
            _lib.check(rc, 'ds_ecp_forces')
            break
        return dict(loc=force[..., 0] if want_walker else None,
                    nl=torch.complex(force[..., 1], force[..., 2]) if want_walker else None,
                    n_bad=n_bad, pairs=pairs, rotations=rot, pair_capacity=cap, sums=sums)

    def energy_stats(self, ke, ew):
        """`ds_energy_stats`: (8,) float64 = [sum Re E_L, sum Im E_L, sum |E_L|^2, n, n_nonfinite, sum Re ke, sum Im ke, sum ew]."""
        out = torch.empty(8, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.ds_energy_stats(self.handle, _ptr(ke), _ptr(ew), ke.shape[0], _ptr(out), _stream()), 'ds_energy_stats')
        return out

    def profile(self, on=True, only=None):
        """Start (and reset) / stop per-kernel HIP-event timing inside the library; `only` = one
        kernel kind of _lib.PROF_KINDS (events around that kernel only)."""
        mode = 0 if not on else (1 if only is None else 2 + _lib.PROF_KINDS.index(only))
        _lib.check(self.lib.ds_profile_enable(self.handle, mode), 'ds_profile_enable')

    def profile_read(self):
        """-> {kernel kind: (total ms, launches)} for the launches since profile(True)."""
        n = len(_lib.PROF_KINDS)
        ms = (C.c_double * n)()
        cnt = (C.c_int64 * n)()
        _lib.check(self.lib.ds_profile_read(self.handle, ms, cnt), 'ds_profile_read')
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(_lib.PROF_KINDS)}

    def int8_layers(self):
        """Number of dense hidden layers per local-energy evaluation whose per-electron contraction runs as an int8 split
        (csrc/ds_i8.h; 0 unless the handle was created with DS_I8=1, or for shapes without an instance)."""
        return int(self.lib.ds_int8_layers(self.handle))

    def pair_recompute_layers(self, dump=False):
        """Number of pair layers per local-energy evaluation (dump: per stage dump) that run the pair layer in front of them in
        registers (k_two_layer_expand<.., PREV>; 0 for a handle created with DS_NO_PAIR_RECOMPUTE=1, in float32, in a stage dump)."""
        return int(self.lib.ds_pair_recompute_layers(self.handle, 1 if dump else 0))

    def profile_clock(self):
        """In-kernel clock probe of the hidden-layer kernel since profile(True): -> (shader cycles, 100 MHz reference ticks,
        GHz) summed over its workgroups; GHz is None when the probe did not run."""
        cyc, ticks = C.c_double(0), C.c_double(0)
        _lib.check(self.lib.ds_profile_read_clock(self.handle, C.byref(cyc), C.byref(ticks)), 'ds_profile_read_clock')
        return cyc.value, ticks.value, (cyc.value / ticks.value * 0.1 if ticks.value > 0 else None)

    def debug_stage(self, params, x, stage, n_elems):
        x = self._check_x(x)
        p = self.pack_params(params)
        ws = self.workspace(x.shape[0])
        out = torch.zeros(int(n_elems), dtype=self.dtype, device=self.device)
        n = self.lib.ds_debug_stage(self.handle, _ptr(p), _ptr(x), x.shape[0], stage.encode(), _ptr(out), out.numel(),
                                    _ptr(ws), ws.numel(), _stream())
        if n < 0:
            raise RuntimeError(f'ds_debug_stage({stage}): {self.lib.ds_last_error().decode()}')
        return out[:n]


def observable_sums(recvec, x, q_int, pol_direction):
    """Batch sums of the walker observables of estimator.py (`ds_observables`, csrc/ds_obs.h); needs no handle.
    recvec (3, 3): the simulation cell's reciprocal vectors (rows g_j); x (B, 3N) float64 / float32 device tensor;
    q_int (Q, 3) integer lattice coordinates in 0..7 (Q may be 0); pol_direction 0..2 or -1 (no polarization).
    -> float64 device tensor [sum Re P, sum Im P, sum Re rho(q_k), sum Im rho(q_k), sum |rho(q_k)|^2] of 2 + 3Q values."""
    _require_gpu()
    if not x.is_cuda:
        raise RuntimeError('observable_sums: walkers must live on the ROCm device (no CPU path)')
    if x.dtype not in _DTYPES:
        raise TypeError(f'observable_sums: walkers must be float64 or float32, got {x.dtype}')
    if x.dim() != 2 or x.shape[1] % 3:
        raise ValueError(f'observable_sums: walkers must have shape (B, 3N), got {tuple(x.shape)}')
    if x.shape[0] < 1:
        raise ValueError('observable_sums: empty walker batch (the observables are batch means)')
    lib = _lib.load()
    x = x.contiguous()
    rv = np.ascontiguousarray(np.asarray(recvec, dtype=np.float64).reshape(3, 3))
    q = np.ascontiguousarray(np.asarray(q_int, dtype=np.int32).reshape(-1, 3))
    B, n_q = x.shape[0], q.shape[0]
    need = lib.ds_observables_workspace_bytes(B, n_q)
    ws = torch.empty(max(int(need), 8) // 8, dtype=torch.float64, device=x.device)
    out = torch.empty(2 + 3 * n_q, dtype=torch.float64, device=x.device)
    _lib.check(lib.ds_observables(_pd(rv), _DTYPES[x.dtype], _ptr(x), B, x.shape[1] // 3,
                                  q.ctypes.data_as(C.POINTER(C.c_int32)), n_q, int(pol_direction), _ptr(out), _ptr(ws),
                                  ws.numel() * 8, _stream()), 'ds_observables')
    return out


def _realspace_setup(who, x, dens, fold_lattice, pair, latvec, r_max, min_rows='B'):
    """What `realspace_counts` and `realspace_counts_w` check alike -> (x contiguous, the host arguments of the C entry in its
    order: fold_inv, grid, latvec, latvec_inv, r_max, n_r)."""
    _require_gpu()
    if not x.is_cuda:
        raise RuntimeError(f'{who}: walkers must live on the ROCm device (no CPU path)')
    if x.dtype not in _DTYPES:
        raise TypeError(f'{who}: walkers must be float64 or float32, got {x.dtype}')
    if x.dim() != 2 or x.shape[1] % 3:
        raise ValueError(f'{who}: walkers must have shape ({min_rows}, 3N), got {tuple(x.shape)}')
    if x.shape[0] < 1:
        raise ValueError(f'{who}: empty walker batch')
    if dens is None and pair is None:
        raise ValueError(f'{who}: neither a density nor a pair buffer was given')
    for name, buf, lead in (('dens', dens, 2), ('pair', pair, 3)):
        if buf is None:
            continue
        if not (isinstance(buf, torch.Tensor) and buf.dtype == torch.int64 and buf.is_contiguous()):
            raise TypeError(f'{who}: {name} must be a contiguous int64 tensor')
        if buf.device != x.device:
            raise RuntimeError(f'{who}: {name} lives on {buf.device}, the walkers on {x.device}')
        if buf.dim() != (4 if lead == 2 else 2) or buf.shape[0] != lead:
            raise ValueError(f'{who}: {name} must have shape ' + ('(2, g0, g1, g2)' if lead == 2 else '(3, n_r)')
                             + f', got {tuple(buf.shape)}')
    f8 = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(3, 3))
    fold_inv = grid = a = a_inv = None
    n_r, rm = 0, 0.0
    if dens is not None:
        if fold_lattice is None:
            raise ValueError(f'{who}: the density needs fold_lattice')
        fold_inv = np.ascontiguousarray(np.linalg.inv(f8(fold_lattice)))
        grid = np.asarray(dens.shape[1:], dtype=np.int32)
    if pair is not None:
        if latvec is None or r_max is None:
            raise ValueError(f'{who}: the pair counts need latvec and r_max')
        a = f8(latvec)
        a_inv = np.ascontiguousarray(np.linalg.inv(a))
        n_r, rm = int(pair.shape[1]), float(r_max)
    keep = (fold_inv, grid, a, a_inv)                      # (the host arrays must outlive the call: the caller holds the tuple)
    args = (_pd(fold_inv) if fold_inv is not None else None, grid.ctypes.data_as(C.POINTER(C.c_int32)) if grid is not None else None,
            _pd(a) if a is not None else None, _pd(a_inv) if a_inv is not None else None, rm, n_r)
    return x.contiguous(), args, keep


def realspace_counts(x, n_up, dens=None, fold_lattice=None, pair=None, latvec=None, r_max=None):
    """Add the real-space counts of the walkers x to caller-owned int64 device buffers (`ds_realspace_counts`,
    csrc/ds_realspace.h); needs no handle, returns nothing and copies nothing to the host.
    x (B, 3N) float64 / float32 device tensor; electrons e < n_up are spin up.
    dens: int64 device tensor (2, g0, g1, g2), the density counts on the grid of `fold_lattice` (3, 3; rows = lattice vectors),
    or None.  pair: int64 device tensor (3, n_r), the up-up / up-down / down-down histogram of minimum-image distances below
    `r_max` in the simulation cell `latvec` (3, 3), or None.  The caller guarantees r_max <= half the shortest lattice vector and
    r_max < 1.5 x the smallest plane spacing (`estimator.RealSpaceAccumulator` checks both)."""
    x, args, keep = _realspace_setup('realspace_counts', x, dens, fold_lattice, pair, latvec, r_max)
    _lib.check(_lib.load().ds_realspace_counts(*args, _DTYPES[x.dtype], _ptr(x), x.shape[0], x.shape[1] // 3, int(n_up), _ptr(dens),
                                               _ptr(pair), _stream()), 'ds_realspace_counts')
    del keep


# ------------------------------------------------------------------ forward walking (csrc/ds_fw.h)
def _fw_array(name, t, dtype, shape, device):
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise ValueError(f'{name} must be a contiguous {dtype} tensor of shape {tuple(shape)}')
    if t.device != device:
        raise RuntimeError(f'{name} lives on {t.device}, expected {device}')
    return t


def dmc_ancestry(parents, anc=None, want_block=False, B=None):
    """`ds_dmc_ancestry`: carry the ancestor tables `anc` (n_slots, B) int32 through one block IN PLACE, given the block's
    `parents` (steps, B) int32 as the DMC step entries write them (None, with `B`: no steps, the identity).  An entry of
    `parents` outside [0, B) loses the lineage: -1, which stays -1.  `anc` None: no tables (only the block map).
    -> the block map P (B,) int32 with `want_block`, else None."""
    _require_gpu()
    ref = parents if parents is not None else anc
    if ref is None:
        if B is None:
            raise ValueError('dmc_ancestry: without parents and tables the number of walkers B is needed')
        dev = torch.device('cuda', torch.cuda.current_device())
    else:
        if not ref.is_cuda:
            raise RuntimeError('dmc_ancestry: parents / anc must live on the ROCm device (no CPU path)')
        if ref.dim() != 2:
            raise ValueError(f'dmc_ancestry: parents must be (steps, B) and anc (n_slots, B), got {tuple(ref.shape)}')
        dev = ref.device
    B = int(ref.shape[1]) if B is None else int(B)
    steps = 0 if parents is None else int(parents.shape[0])
    n_slots = 0 if anc is None else int(anc.shape[0])
    _fw_array('dmc_ancestry: parents', parents, torch.int32, (steps, B), dev)
    _fw_array('dmc_ancestry: anc', anc, torch.int32, (n_slots, B), dev)
    lib = _lib.load()
    need = int(lib.ds_dmc_ancestry_workspace_bytes(B, n_slots))
    ws = torch.empty(max(need, 4) // 4, dtype=torch.int32, device=dev)
    block = torch.empty(B, dtype=torch.int32, device=dev) if want_block else None
    _lib.check(lib.ds_dmc_ancestry(B, steps, _ptr(parents), n_slots, _ptr(anc), _ptr(block), _ptr(ws), ws.numel() * 4, _stream()),
               'ds_dmc_ancestry')
    return block


def realspace_counts_w(x, n_up, q_sum, n_bad, index=None, weight=None, weight_scale=1.0, dens=None, fold_lattice=None, pair=None,
                       latvec=None, r_max=None):
    """`ds_realspace_counts_w`: `realspace_counts` with a source row and an integer weight per walker.  Walker w adds the
    positions of row `index[w]` (int32 (B,); None: row w) of x (B_src, 3N) with the weight q = rint(weight[w] * weight_scale)
    (`weight` float64 (B,); None: 1) to the int64 buffers `dens` / `pair`; q_sum (1,) int64 += sum q; n_bad (2,) int64 += the
    walkers skipped for their index / for their weight (not finite, negative, q > 2^24).  Nothing is zeroed or copied to the host."""
    x, args, keep = _realspace_setup('realspace_counts_w', x, dens, fold_lattice, pair, latvec, r_max, min_rows='B_src')
    B = int(index.shape[0]) if index is not None else (int(weight.shape[0]) if weight is not None else int(x.shape[0]))
    if q_sum is None or n_bad is None:
        raise ValueError('realspace_counts_w: q_sum and n_bad are needed')
    _fw_array('realspace_counts_w: index', index, torch.int32, (B,), x.device)
    _fw_array('realspace_counts_w: weight', weight, torch.float64, (B,), x.device)
    _fw_array('realspace_counts_w: q_sum', q_sum, torch.int64, (1,), x.device)
    _fw_array('realspace_counts_w: n_bad', n_bad, torch.int64, (2,), x.device)
    _lib.check(_lib.load().ds_realspace_counts_w(*args, _DTYPES[x.dtype], _ptr(x), B, x.shape[1] // 3, int(n_up), _ptr(dens), _ptr(pair),
                                                 int(x.shape[0]), _ptr(index), _ptr(weight), float(weight_scale), _ptr(q_sum),
                                                 _ptr(n_bad), _stream()), 'ds_realspace_counts_w')
    del keep


def dmc_fw_sums(values, index=None, weight=None, n_bad=None):
    """`ds_dmc_fw_sums`: out[k] = (sum_w weight[w] values[index[w], k], sum_w weight[w]) over the walkers with a valid index, a
    finite weight > 0 and a finite value, in the fixed summation order of the DMC stats rows.  values (B_src, K) float64; index
    (B,) int32 or None (row w); weight (B,) float64 or None (1); n_bad (2,) int64, added to (None: a fresh one).
    -> (out (K, 2) float64 device tensor, n_bad)."""
    _require_gpu()
    if not (isinstance(values, torch.Tensor) and values.is_cuda and values.dtype == torch.float64 and values.dim() == 2):
        raise ValueError('dmc_fw_sums: values must be a (B_src, K) float64 tensor on the ROCm device (no CPU path)')
    values = values.contiguous()
    B_src, K = (int(v) for v in values.shape)
    B = int(index.shape[0]) if index is not None else (int(weight.shape[0]) if weight is not None else B_src)
    _fw_array('dmc_fw_sums: index', index, torch.int32, (B,), values.device)
    _fw_array('dmc_fw_sums: weight', weight, torch.float64, (B,), values.device)
    if n_bad is None:
        n_bad = torch.zeros(2, dtype=torch.int64, device=values.device)
    _fw_array('dmc_fw_sums: n_bad', n_bad, torch.int64, (2,), values.device)
    lib = _lib.load()
    need = int(lib.ds_dmc_fw_sums_workspace_bytes(B, K))
    ws = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=values.device)
    out = torch.empty(max(K, 1), 2, dtype=torch.float64, device=values.device)
    _lib.check(lib.ds_dmc_fw_sums(B, K, _ptr(values), B_src, _ptr(index), _ptr(weight), _ptr(out), _ptr(n_bad), _ptr(ws),
                                  ws.numel() * 8, _stream()), 'ds_dmc_fw_sums')
    return out, n_bad


class HfOrbitalTables:
    """The device tables of one `hf.GaussianOrbitals` (`ds_hf_create`, csrc/ds_hf.h); needs no DeviceSystem.  The arrays are
    the fields of `ds_hf_desc` (include/deepsolid_hip.h); `mo` is the pair of (nao, n_s) complex128 coefficient matrices."""

    def __init__(self, a, atoms, shell_atom, shell_l, shell_nprim, exps, coefs, kpts, images, nocc, mo, device=None):
        _require_gpu()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        f8 = lambda v, shape: np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(shape))
        i4 = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.int32).reshape(-1))
        pi = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))
        a, atoms, kpts, images = f8(a, (3, 3)), f8(atoms, (-1, 3)), f8(kpts, (-1, 3)), f8(images, (-1, 3))
        shell_atom, shell_l, shell_nprim = i4(shell_atom), i4(shell_l), i4(shell_nprim)
        exps, coefs = f8(exps, -1), f8(coefs, -1)
        nocc = [i4(n) for n in nocc]
        mo = [np.ascontiguousarray(np.asarray(m, dtype=np.complex128)) for m in mo]
        self.nelec = tuple(int(m.shape[1]) for m in mo)
        d = _lib.HfDesc()
        d.a[:] = a.reshape(-1).tolist()
        d.n_atoms, d.atoms = atoms.shape[0], _pd(atoms)
        d.n_shells, d.shell_atom, d.shell_l, d.shell_nprim = shell_l.shape[0], pi(shell_atom), pi(shell_l), pi(shell_nprim)
        d.exps, d.coefs = _pd(exps), _pd(coefs)
        d.n_k, d.kpts = kpts.shape[0], _pd(kpts)
        d.n_images, d.images = images.shape[0], _pd(images)
        d.n_up, d.n_dn = self.nelec
        d.nocc_up, d.nocc_dn = pi(nocc[0]), pi(nocc[1])
        d.mo_up, d.mo_dn = (m.view(np.float64).ctypes.data_as(C.POINTER(C.c_double)) if m.size else None for m in mo)
        self.handle = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ds_hf_create(C.byref(d), C.byref(self.handle)), 'ds_hf_create')

    def __del__(self):
        h, self.handle = getattr(self, 'handle', None), None
        if h:
            try:
                self.lib.ds_hf_destroy(h)
            except Exception:
                pass

    def orbitals(self, x):
        """x (B, 3N) float64 / float32 device tensor -> [up (B, n_up, n_up), dn (B, n_dn, n_dn)] complex128 (`ds_hf_orbitals`)."""
        if not x.is_cuda or x.device != self.device:
            raise RuntimeError(f'HfOrbitalTables.orbitals: walkers must live on {self.device} (no CPU path)')
        if x.dtype not in _DTYPES:
            raise TypeError(f'HfOrbitalTables.orbitals: walkers must be float64 or float32, got {x.dtype}')
        n = sum(self.nelec)
        if x.dim() != 2 or x.shape[1] != 3 * n:
            raise ValueError(f'HfOrbitalTables.orbitals: walkers must have shape (B, {3 * n}), got {tuple(x.shape)}')
        x = x.contiguous()
        B = x.shape[0]
        outs = [torch.empty(B, ns, ns, 2, dtype=torch.float64, device=x.device) for ns in self.nelec]
        if B:
            with torch.cuda.device(self.device):
                _lib.check(self.lib.ds_hf_orbitals(self.handle, _DTYPES[x.dtype], _ptr(x), B, _ptr(outs[0] if self.nelec[0] else None),
                                                   _ptr(outs[1] if self.nelec[1] else None), _stream()), 'ds_hf_orbitals')
        return [torch.view_as_complex(o) for o in outs]

    def _points_like(self, what, t, shape_tail):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == self.device):
            raise RuntimeError(f'HfOrbitalTables.{what} must live on {self.device} (no CPU path)')
        if t.dtype not in _DTYPES:
            raise TypeError(f'HfOrbitalTables.{what} must be float64 or float32, got {t.dtype}')
        if tuple(t.shape[t.dim() - len(shape_tail):]) != tuple(shape_tail) or t.dim() != len(shape_tail) + 1:
            raise ValueError(f'HfOrbitalTables.{what} must have shape (*, {", ".join(str(v) for v in shape_tail)}), got {tuple(t.shape)}')
        return t.contiguous()

    def orbitals_at(self, points, spin):
        """points (P, 3) float64 / float32 device tensor -> (P, M_spin) complex128: the orbitals of ONE spin at arbitrary points
        (`ds_hf_orbitals_at`); at an electron's position the bits are those of `orbitals`.  A spin without orbitals gives (P, 0)."""
        spin = int(spin)
        if spin not in (0, 1):
            raise ValueError(f'HfOrbitalTables.orbitals_at: spin must be 0 or 1, got {spin}')
        points = self._points_like('orbitals_at: points', points, (3,))
        P, ns = int(points.shape[0]), self.nelec[spin]
        out = torch.empty(P, ns, 2, dtype=torch.float64, device=self.device)
        if P and ns:
            with torch.cuda.device(self.device):
                _lib.check(self.lib.ds_hf_orbitals_at(self.handle, spin, _DTYPES[points.dtype], _ptr(points), P, _ptr(out), _stream()),
                           'ds_hf_orbitals_at')
        return torch.view_as_complex(out) if ns else torch.empty(P, 0, dtype=torch.complex128, device=self.device)

    def obdm_accumulate(self, x, nelec, n_samples, first_electron, ratios, shifts, weights=None, dm_sums=None, ov_sums=None,
                        max_bytes=None):
        """`ds_obdm_accumulate`: fold the ratios q (B, M) complex (or (B, M, 2) real) and shifts (B, M, 3) that
        `DeviceSystem.one_body_ratios(..., want_ratios=True, want_shifts=True)` exports for the walkers x (B, 3N), N = sum(nelec),
        into the sums of the one-body density matrix in this basis (include/deepsolid_hip.h):
            dm_sums[s][i][j] += w q conj(phi_i(r')) phi_j(r_e),      ov_sums[s][i][j] += w conj(phi_i(r')) phi_j(r').
        x, ratios and shifts share one dtype (float64 or float32); `weights` (B, M) float64 or None (1).  `dm_sums` / `ov_sums`:
        float64 device tensors (2, Mb, Mb, 2), Mb = max(M_up, M_dn), ADDED to (None: fresh zero ones).  `max_bytes` caps the
        workspace: more chunks, bit-identical sums.  -> dict(dm_sums, ov_sums, n_bad (2,) int64 device tensor: samples left out
        because q or the weight was not finite).  No host synchronisation."""
        x = self._points_like('obdm_accumulate: walkers', x, (3 * (int(nelec[0]) + int(nelec[1])),))
        B, M, N = int(x.shape[0]), int(n_samples), int(nelec[0]) + int(nelec[1])
        if ratios.is_complex():
            ratios = torch.view_as_real(ratios)
        ratios = self._points_like('obdm_accumulate: ratios', ratios, (M, 2))
        shifts = self._points_like('obdm_accumulate: shifts', shifts, (M, 3))
        if ratios.dtype != x.dtype or shifts.dtype != x.dtype or ratios.shape[0] != B or shifts.shape[0] != B:
            raise ValueError(f'obdm_accumulate: ratios ({B}, {M}, 2) and shifts ({B}, {M}, 3) must have the walkers\' dtype {x.dtype}')
        if weights is not None:
            if not (weights.is_cuda and weights.dtype == torch.float64 and tuple(weights.shape) == (B, M)):
                raise ValueError(f'obdm_accumulate: weights must be a float64 device tensor of shape ({B}, {M})')
            weights = weights.contiguous()
        Mb = max(self.nelec)
        sums = []
        for name, t in (('dm_sums', dm_sums), ('ov_sums', ov_sums)):
            if t is None:
                t = torch.zeros(2, Mb, Mb, 2, dtype=torch.float64, device=self.device)
            elif not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (2, Mb, Mb, 2)):
                raise ValueError(f'obdm_accumulate: {name} must be a contiguous float64 device tensor of shape (2, {Mb}, {Mb}, 2)')
            sums.append(t)
        n_bad = torch.zeros(2, dtype=torch.int64, device=self.device)
        need = int(self.lib.ds_obdm_workspace_bytes(self.handle, B, M))
        if need < 0:
            raise ValueError(f'obdm_accumulate: B = {B} and n_samples = {M} must be >= 1')
        if max_bytes is not None:
            need = min(need, int(max_bytes))
        ws = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ds_obdm_accumulate(self.handle, _DTYPES[x.dtype], _ptr(x), B, N, int(nelec[0]), M, int(first_electron),
                                                   _ptr(ratios), _ptr(shifts), _ptr(weights), _ptr(sums[0]), _ptr(sums[1]),
                                                   _ptr(n_bad), _ptr(ws), ws.numel() * 8, _stream()), 'ds_obdm_accumulate')
        return dict(dm_sums=sums[0], ov_sums=sums[1], n_bad=n_bad)


class EcpTables:
    """The device tables of one `pseudopotential.SemiLocalECP` (`ds_ecp_create`, csrc/ds_ecp.h): the fields of `ds_ecp_desc`
    (include/deepsolid_hip.h).  The library repeats the checks of `SemiLocalECP` (cutoffs, n_quad, n_l, term tables)."""

    def __init__(self, ecp, device=None):
        _require_gpu()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.ecp = ecp
        self.n_quad = int(ecp.n_quad)
        d, self._keep = ecp_desc(ecp)
        self.handle = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ds_ecp_create(C.byref(d), C.byref(self.handle)), 'ds_ecp_create')

    def __del__(self):
        h, self.handle = getattr(self, 'handle', None), None
        if h:
            try:
                self.lib.ds_ecp_destroy(h)
            except Exception:
                pass


def ecp_desc(ecp, **override):
    """-> (`_lib.EcpDesc` of a `pseudopotential.SemiLocalECP`, the host arrays it points to: keep them alive as long as the
    descriptor).  `override` replaces fields (arrays or scalars) by name: the refusal tests of the C ABI."""
    f8 = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    i4 = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.int32).reshape(-1))
    t = ecp.tables()
    arrays = dict(atoms=f8(ecp.atoms), atom_species=i4(ecp.atom_species), n_l=i4(ecp.n_l), r_cut_loc=f8(ecp.r_cut_loc),
                  r_cut_nl=f8(ecp.r_cut_nl), term_offset=i4(t['term_offset']), term_n=i4(t['term_n']), term_zeta=f8(t['term_zeta']),
                  term_c=f8(t['term_c']))
    scalars = dict(a=f8(ecp.a), n_atoms=len(ecp.atoms), n_species=ecp.n_species, n_quad=ecp.n_quad)
    for k, v in override.items():
        if k in arrays:
            arrays[k] = (f8 if arrays[k].dtype == np.float64 else i4)(v)
        else:
            scalars[k] = f8(v) if k == 'a' else int(v)
    d = _lib.EcpDesc()
    d.a[:] = scalars['a'].tolist()
    d.n_atoms, d.n_species, d.n_quad = scalars['n_atoms'], scalars['n_species'], scalars['n_quad']
    for k, v in arrays.items():
        setattr(d, k, v.ctypes.data_as(C.POINTER(C.c_double if v.dtype == np.float64 else C.c_int32)))
    return d, arrays

"""The map between a reference parameter tree (network.py:135-186) and the flat device buffer of `ds_param_layout`
(include/deepsolid_hip.h), as data: ONE integer gather vector per tree shape.  Packing, unpacking a packed gradient and the
KFAC index are each one gather with it.  Nothing here needs a GPU or a library handle.
"""
from types import SimpleNamespace

import numpy as np
import torch


def _walk(o, out, path):
    """The one tree walk, in the reference's order (dict keys sorted, lists and tuples in order): appends every leaf to `out`,
    as (path, leaf) when a `path` tuple is carried along."""
    if isinstance(o, dict):
        for k in sorted(o):
            _walk(o[k], out, path and path + (k,))
    elif isinstance(o, (list, tuple)):
        for i, v in enumerate(o):
            _walk(v, out, path and path + (i,))
    else:
        out.append((path[1:], o) if path else o)
    return out


def _shape(leaf):
    return tuple(leaf.shape) if isinstance(leaf, torch.Tensor) else np.shape(leaf)


def tree_leaves(tree):
    """The leaves of a parameter tree in the reference's order: dict keys sorted, lists and tuples in order."""
    return _walk(tree, [], None)


def tree_like(tree, flat):
    """Cut the flat vector `flat` into leaves shaped like those of `tree` (dicts stay dicts, lists and tuples become lists)."""
    off = [0]

    def build(o):
        if isinstance(o, dict):
            return {k: build(o[k]) for k in sorted(o)}
        if isinstance(o, (list, tuple)):
            return [build(v) for v in o]
        n = int(np.prod(_shape(o), dtype=np.int64))
        off[0] += n
        return flat[off[0] - n:off[0]].reshape(_shape(o))
    return build(tree)


def orbital_column_map(nparam, cols, dtype):
    """Packed column c -> reference column of orbital[s]['w'] (or -1 for zero padding).
    Within every 16-column tile t the MFMA accumulator gives lane group q = lane >> 4 the rows
    {q, q+4, q+8, q+12} (f64) or {4q .. 4q+3} (f32) in registers r = 0..3; they are assigned
    (Re p, Im p, Re p+4, Im p+4) with p = 8t + q, so the complex product with the envelope/phase jet
    is lane-local in the fused orbital epilogue (csrc/ds_gemm.h: orb_col)."""
    src = -np.ones(cols, dtype=np.int64)
    for t in range(cols // 16):
        for q in range(4):
            for r in range(4):
                row = q + 4 * r if dtype == torch.float64 else 4 * q + r
                p = 8 * t + q + 4 * (r // 2)
                if p < nparam:
                    src[16 * t + row] = p + (r % 2) * nparam
    return src


def _pad(m, axis, size):
    """`m` with -1 entries (zero padding of the buffer) appended along `axis` up to `size`."""
    width = [(0, 0)] * m.ndim
    width[axis] = (0, size - m.shape[axis])
    return np.pad(m, width, constant_values=-1)


class ParamMap:
    """Layout of the parameter buffer for one architecture.

    `nelec`: (n_up, n_dn) after the mirroring of a spin-down-only cell; `hidden_dims`: the reference's widths, `device_dims` the
    padded ones the kernels run (`device.device_plan`); `natom`: atoms of the primitive cell; `envelope_type`: kept for the
    record, sigma's rows follow from its shape; `dtype`: element type of the buffer (the orbital column map differs between
    float64 and float32); `blocks`: [(offset, rows, cols)] of `ds_param_layout`; `param_count`: elements of the buffer.

    `layout(params)`, built once per tree shape, holds the int64 numpy vectors `gather` (length `param_count`: position i holds
    the tree-flat entry index -- leaves in `tree_leaves` order, row-major -- that lands at packed position i, -1 where the buffer
    is zero padding) and `pos` (its inverse: the packed position of every tree entry, -1 for an entry without a place)."""

    def __init__(self, nelec, n_det, hidden_dims, device_dims, natom, distance_type, envelope_type, full_det, use_last_layer,
                 bias_orbitals, dtype, blocks, param_count):
        self.nelec, self.n_det = tuple(nelec), int(n_det)
        self.hidden_dims, self.device_dims = tuple(hidden_dims), tuple(device_dims)
        self.natom, self.distance_type, self.envelope_type = int(natom), distance_type, envelope_type
        self.full_det, self.use_last_layer, self.bias_orbitals = bool(full_det), bool(use_last_layer), bool(bias_orbitals)
        self.dtype = dtype
        self.blocks = [tuple(int(v) for v in b) for b in blocks]
        self.param_count = int(param_count)
        self._layouts = {}
        self._packed, self._packed_key, self._packed_leaves = None, None, []

    def layout(self, params):
        """-> namespace(gather, pos, idx: {leaf path: its entries' tree-flat indices, shaped like the leaf}, dev: tensor cache)."""
        items = _walk(params, [], (None,))
        key = tuple((path, _shape(leaf)) for path, leaf in items)
        if key not in self._layouts:
            idx, total = {}, 0
            for path, shape in key:
                n = int(np.prod(shape, dtype=np.int64))
                idx[path] = np.arange(total, total + n, dtype=np.int64).reshape(shape)
                total += n
            gather = self._gather(idx)
            placed = np.nonzero(gather >= 0)[0]
            pos = np.full(total, -1, dtype=np.int64)
            pos[gather[placed]] = placed
            self._layouts[key] = SimpleNamespace(gather=gather, pos=pos, idx=idx, dev={})
        return self._layouts[key]

    def _gather(self, idx):
        """What packing does to the values, done to the entries' own numbers `idx`."""
        nch = 2 if self.nelec[1] > 0 else 1
        n_layers, n_double = len(self.hidden_dims), len(self.hidden_dims) - (0 if self.use_last_layer else 1)
        need = 3 * n_layers + 2 * n_double + nch * (3 + self.use_last_layer + self.bias_orbitals)
        if len(self.blocks) != need:
            raise ValueError(f'the parameter layout holds {len(self.blocks)} blocks, this architecture needs {need}')
        gather = np.full(self.param_count, -1, dtype=np.int64)
        bi = iter(self.blocks)

        def put(mat):
            off, rows, cols = next(bi)
            mat = mat.reshape(rows, cols) if mat.size == rows * cols else mat
            if tuple(mat.shape) != (rows, cols):
                raise ValueError(f'parameter block shape {tuple(mat.shape)} != expected {(rows, cols)}')
            gather[off:off + rows * cols] = mat.reshape(-1)
        nf = 4 if self.distance_type == 'nu' else 7
        r4 = lambda v: (v + 3) // 4 * 4
        # reference widths (network.py:111-132) and the device widths (layer-0 rows padded to the MFMA k-step, hidden widths
        # to what the kernels run: device_widths)
        h1_ref = [nf * self.natom] + [h[0] for h in self.hidden_dims]
        h2_ref = [nf] + [h[1] for h in self.hidden_dims]
        h1 = [r4(nf * self.natom)] + [h[0] for h in self.device_dims]
        h2 = [r4(nf)] + [h[1] for h in self.device_dims]

        def split(w, l):
            """Rows [h | mean_up | mean_dn | m2_up | m2_dn] of a layer-l input (network.py:126-128) -> per-electron rows
            [h | m2_up | m2_dn] and shared rows [mean_up | mean_dn], every segment padded to its device width."""
            kh, k2 = h1_ref[l], h2_ref[l]
            m2 = [_pad(w[(nch + 1) * kh + c * k2:(nch + 1) * kh + (c + 1) * k2], 0, h2[l]) for c in range(nch)]
            return (np.concatenate([_pad(w[:kh], 0, h1[l])] + m2, axis=0),
                    np.concatenate([_pad(w[(1 + c) * kh:(2 + c) * kh], 0, h1[l]) for c in range(nch)], axis=0))
        for l in range(n_layers):
            w = idx['single', l, 'w']
            want = ((nch + 1) * h1_ref[l] + nch * h2_ref[l], h1_ref[l + 1])
            if tuple(w.shape) != want:
                raise ValueError(f"single[{l}]['w'] has shape {tuple(w.shape)}, expected {want}")
            for part in split(_pad(w, 1, h1[l + 1]), l):
                put(part)
            put(_pad(idx['single', l, 'b'].reshape(1, -1), 1, h1[l + 1]))
        for l in range(n_double):
            put(_pad(_pad(idx['double', l, 'w'], 0, h2[l]), 1, h2[l + 1]))
            put(_pad(idx['double', l, 'b'].reshape(1, -1), 1, h2[l + 1]))
        for c in range(nch):
            nparam = (sum(self.nelec) if self.full_det else self.nelec[c]) * self.n_det
            w = idx['orbital', c, 'w']
            if w.shape[1] != 2 * nparam:
                raise ValueError(f"orbital[{c}]['w'] has {w.shape[1]} columns, expected {2 * nparam}")
            for part in split(w, n_layers) if self.use_last_layer else [_pad(w, 0, h1[-1])]:
                off, rows, cols = next(bi)
                if part.shape[0] != rows:
                    raise ValueError(f"orbital[{c}]['w'] block has {part.shape[0]} rows, expected {rows}")
                src = orbital_column_map(nparam, cols, self.dtype)
                gather[off:off + rows * cols] = np.where(src >= 0, part[:, src], -1).reshape(-1)
            if self.bias_orbitals:
                put(idx['orbital', c, 'b'])
            put(idx['envelope', c, 'pi'])
            # sigma: (A, P) isotropic | (A, 3, P) diagonal -> rows a*3+c | (3, 3, A, P) full -> rows (k*3+m)*A+a
            put(idx['envelope', c, 'sigma'].reshape(-1, nparam))
        return gather

    @staticmethod
    def _on(lay, name, device):
        """`gather` (its padding pointing at the zero appended behind the tree-flat vector) or `pos` as a tensor on `device`."""
        if (name, device) not in lay.dev:
            if name == 'pos' and (lay.pos < 0).any():
                raise RuntimeError('parameter entries without a place in the packed buffer')
            v = lay.pos if name == 'pos' else np.where(lay.gather < 0, lay.pos.size, lay.gather)
            lay.dev[name, device] = torch.as_tensor(v).to(device)
        return lay.dev[name, device]

    def pack(self, params, device, dtype):
        """Parameter tree -> the flat buffer on `device` in `dtype`.  Cached on the leaves' versions."""
        leaves = tree_leaves(params)
        # cache only trees of tensors: the key holds the leaves themselves (so ids cannot be recycled), their
        # storage address and version counter; numpy leaves have no version counter and are packed every call
        cacheable = all(isinstance(t, torch.Tensor) for t in leaves)
        key = (device, dtype) + tuple((t.data_ptr(), t._version) for t in leaves) if cacheable else None
        if cacheable and self._packed is not None and key == self._packed_key and \
                len(leaves) == len(self._packed_leaves) and all(a is b for a, b in zip(leaves, self._packed_leaves)):
            return self._packed
        vals = [(t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))).to(device=device, dtype=dtype).reshape(-1)
                for t in leaves]
        flat = torch.cat(vals + [torch.zeros(1, dtype=dtype, device=device)])
        flat = flat.index_select(0, self._on(self.layout(params), 'gather', device))
        self._packed, self._packed_key, self._packed_leaves = (flat, key, leaves) if cacheable else (None, None, [])
        return flat

    def unpack(self, flat, params):
        """Packed vector (a gradient) -> a tree shaped like `params`."""
        return tree_like(params, flat[self._on(self.layout(params), 'pos', flat.device)])

    def kfac_index(self, layout, params, device='cpu'):
        """Index maps of the KFAC step for a tree shaped like `params` and the block dicts `layout` of `kfac_layout()`, built once:
        -> dict(v_src, diag_src: positions in the PACKED buffer of every entry of v (all blocks' d_in x d_out matrices in layout
        order, rows in the reference's order w.reshape(-1, d_out) then b) and of the untagged leaves (envelope pi, sigma);
        v_tree, diag_tree: the same entries as positions in the tree-flat vector; leaf_sizes: entries per leaf of that vector;
        diag_paths: the untagged leaves).  Packing is `packed.index_select(0, v_src)`, unpacking one `index_copy_`."""
        lay = self.layout(params)
        if ('kfac', device) in lay.dev:
            return lay.dev['kfac', device]
        pos = self._on(lay, 'pos', device)
        tagged = []
        for b in layout:
            w = lay.idx[b['kind'], b['index'], 'w']
            d_out = w.shape[-1]
            rows = w.size // d_out + (1 if b['has_bias'] else 0)
            if d_out != b['d_out'] or rows != b['d_in']:
                raise ValueError(f"{b['kind']}[{b['index']}]: the tree holds a {rows} x {d_out} block, the layout {b['d_in']} x {b['d_out']}")
            if b['has_bias'] and lay.idx[b['kind'], b['index'], 'b'].size != d_out:
                raise ValueError(f"{b['kind']}[{b['index']}]['b'] does not have {d_out} entries")
            tagged += [(b['kind'], b['index'], k) for k in (('w', 'b') if b['has_bias'] else ('w',))]
        diag_paths = [p for p in lay.idx if p not in tagged]

        def entries(paths):
            return torch.as_tensor(np.concatenate([lay.idx[p].reshape(-1) for p in paths] + [np.zeros(0, dtype=np.int64)])).to(device)
        v_tree, diag_tree = entries(tagged), entries(diag_paths)
        lay.dev['kfac', device] = dict(v_src=pos[v_tree], diag_src=pos[diag_tree], v_tree=v_tree, diag_tree=diag_tree,
                                       leaf_sizes=[a.size for a in lay.idx.values()], diag_paths=diag_paths)
        return lay.dev['kfac', device]

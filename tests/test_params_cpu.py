"""CPU checks of deepsolid_amd/params.py: the map between a parameter tree and the flat buffer of `ds_param_layout`.

The expected gather vectors of tests/golden/param_map.npz were recorded from the packing code this module replaced
(`DeviceSystem.pack_params` and the inverse it derived by packing a numbered tree), driven on CPU tensors with the blocks laid out
by the rule of include/deepsolid_hip.h (`param_map_helpers.header_blocks`; tests/test_gpu_workspace.py holds that rule to
`ds_param_layout` of a real handle).  One case per branch of the builder, each in float64 and float32; for the default-width LiH
and bcc-Li trees only the SHA-256 of the int64 gather bytes is stored.  `device_plan` is host code of the library, so the library
must be built."""
import hashlib
import os

import numpy as np
import pytest
import torch

import kfac_step_helpers as ks
import param_map_helpers as H
from deepsolid_amd.params import ParamMap, tree_leaves, tree_like

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'param_map.npz'))
CASE_DTYPES = [(name, tag) for name in H.CASES for tag in H.DTYPES]


@pytest.fixture(scope='module', autouse=True)
def library():
    from deepsolid_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def numbered(tree):
    """The tree with entry k of the tree-flat vector holding k + 1, in float64."""
    total = sum(t.numel() for t in tree_leaves(tree))
    return tree_like(tree, torch.arange(1, total + 1, dtype=torch.float64))


@pytest.mark.parametrize('name,tag', CASE_DTYPES)
def test_gather_equals_the_recorded_layout(name, tag):
    pm, cell, net_kw = H.param_map(name, H.DTYPES[tag])
    assert np.array_equal(np.asarray(pm.blocks), GOLDEN[f'{name}_blocks'])
    assert pm.param_count == int(GOLDEN[f'{name}_param_count'])
    gather = pm.layout(H.make_tree(cell, net_kw)).gather
    assert gather.dtype == np.int64 and gather.shape == (pm.param_count,)
    assert np.array_equal(gather, GOLDEN[f'{name}_{tag}_gather'])


@pytest.mark.parametrize('tag', list(H.DTYPES))
@pytest.mark.parametrize('name', list(H.DIGEST_CASES))
def test_gather_digest_of_the_default_trees(name, tag):
    pm, cell, net_kw = H.param_map(name, H.DTYPES[tag])
    assert pm.param_count == int(GOLDEN[f'{name}_param_count'])
    gather = np.ascontiguousarray(pm.layout(H.make_tree(cell, net_kw)).gather, dtype=np.int64)
    assert hashlib.sha256(gather.tobytes()).hexdigest() == str(GOLDEN[f'{name}_{tag}_sha256'])


@pytest.mark.parametrize('name,tag', CASE_DTYPES)
def test_numbered_tree_packs_to_gather_and_every_entry_has_one_place(name, tag):
    pm, cell, net_kw = H.param_map(name, H.DTYPES[tag])
    tree = H.make_tree(cell, net_kw)
    gather = pm.layout(tree).gather
    packed = pm.pack(numbered(tree), 'cpu', torch.float64)         # float64 carries the numbers in a float32 layout too
    assert torch.equal(packed, torch.as_tensor(gather + 1).double())
    total = sum(t.numel() for t in tree_leaves(tree))
    assert np.array_equal(np.sort(gather[gather >= 0]), np.arange(total))
    pos = pm.layout(tree).pos
    assert pos.shape == (total,) and np.array_equal(gather[pos], np.arange(total))


@pytest.mark.parametrize('name,tag', CASE_DTYPES)
def test_unpack_inverts_pack_bit_for_bit(name, tag):
    dtype = H.DTYPES[tag]
    pm, cell, net_kw = H.param_map(name, dtype)
    tree = H.make_tree(cell, net_kw, dtype=dtype)
    packed = pm.pack(tree, 'cpu', dtype)
    assert packed.dtype == dtype and packed.shape == (pm.param_count,)
    back = pm.unpack(packed, tree)
    assert sorted(back) == sorted(tree) and all(len(back[k]) == len(tree[k]) for k in tree)
    for a, b in zip(tree_leaves(back), tree_leaves(tree)):
        assert a.shape == b.shape and torch.equal(a, b)
    assert bool((packed[torch.as_tensor(pm.layout(tree).gather < 0)] == 0).all())


@pytest.mark.parametrize('name', list(H.CASES))
def test_float32_pack_is_the_float64_pack_rounded(name):
    """The leaves are rounded one by one, then gathered: the same bits as rounding the float64 buffer of the same layout."""
    pm, cell, net_kw = H.param_map(name, torch.float32)
    tree = H.make_tree(cell, net_kw)
    assert torch.equal(pm.pack(tree, 'cpu', torch.float32), pm.pack(tree, 'cpu', torch.float64).float())


def test_packed_buffer_cache():
    pm, cell, net_kw = H.param_map('lih_plain', torch.float64)
    tree = H.make_tree(cell, net_kw)
    first = pm.pack(tree, 'cpu', torch.float64)
    assert pm.pack(tree, 'cpu', torch.float64) is first                       # same leaves, same versions: the same object
    leaf = tree['single'][1]['b']
    leaf.add_(1)                                                               # in place: what train.adam and kfac do
    second = pm.pack(tree, 'cpu', torch.float64)
    assert second is not first and not torch.equal(second, first)
    assert torch.equal(pm.unpack(second, tree)['single'][1]['b'], leaf)
    assert pm.pack(tree, 'cpu', torch.float64) is second
    same_values = {k: [dict(d) for d in v] for k, v in tree.items()}
    same_values['single'][0]['w'] = tree['single'][0]['w'].clone()             # another leaf object: not the cached tree
    third = pm.pack(same_values, 'cpu', torch.float64)
    assert third is not second and torch.equal(third, second)
    nptree = {k: [{kk: vv.numpy().copy() for kk, vv in d.items()} for d in v] for k, v in tree.items()}
    a = pm.pack(nptree, 'cpu', torch.float64)
    nptree['single'][1]['b'] += 1.0                                            # numpy leaves carry no version: never cached
    b = pm.pack(nptree, 'cpu', torch.float64)
    assert a is not b and torch.equal(a, second) and not torch.equal(b, a)
    assert pm.pack(tree, 'cpu', torch.float64) is not second                   # (and they evict the cached buffer, as before)


def test_mis_shaped_trees_and_layouts_raise():
    pm, cell, net_kw = H.param_map('lih_plain', torch.float64)
    tree = H.make_tree(cell, net_kw)

    def changed(kind, i, key, value):
        out = {k: [dict(d) for d in v] for k, v in tree.items()}
        out[kind][i][key] = value
        return out
    with pytest.raises(ValueError, match=r"single\[1\]\['w'\] has shape \(223, 64\), expected \(224, 64\)"):
        pm.pack(changed('single', 1, 'w', torch.zeros(223, 64)), 'cpu', torch.float64)
    with pytest.raises(ValueError, match=r"orbital\[0\]\['w'\] has 30 columns, expected 32"):
        pm.pack(changed('orbital', 0, 'w', torch.zeros(64, 30)), 'cpu', torch.float64)
    with pytest.raises(ValueError, match=r'parameter block shape \(2, 15\) != expected \(2, 16\)'):
        pm.layout(changed('envelope', 0, 'pi', torch.zeros(2, 15)))
    a = H.arch(cell, net_kw)
    blocks, count = H.header_blocks(a)
    wrong = list(blocks)
    wrong[3] = (wrong[3][0], wrong[3][1], wrong[3][2] - 1)
    with pytest.raises(ValueError, match=r'parameter block shape \(\d+, \d+\) != expected \(\d+, \d+\)'):
        ParamMap(dtype=torch.float64, blocks=wrong, param_count=count, **a).layout(tree)
    for short in (blocks[:-1], blocks[:5] + blocks[6:]):          # one block short: never a silent mis-assignment
        with pytest.raises(ValueError, match='the parameter layout holds 13 blocks, this architecture needs 14'):
            ParamMap(dtype=torch.float64, blocks=short, param_count=count, **a).layout(tree)
    extra = changed('double', 0, 'unused', torch.zeros(3))          # packs (the leaf is not read) but has no way back
    pm.pack(extra, 'cpu', torch.float64)
    with pytest.raises(RuntimeError, match='parameter entries without a place in the packed buffer'):
        pm.unpack(torch.zeros(pm.param_count), extra)


def hand_layout(rows):
    """The dict form of `DeviceSystem.kfac_layout()` from (kind, index, has_bias, d_in, d_out, repeats) rows."""
    out, off = [], 0
    for kind, index, has_bias, d_in, d_out, repeats in rows:
        out.append(dict(kind=kind, index=index, param_blocks=[], has_bias=has_bias, d_in=d_in, d_out=d_out, repeats=repeats,
                        a_offset=off, g_offset=off + d_in * d_in))
        off += d_in * d_in + d_out * d_out
    return out


# LiH (2 + 2 electrons, two atoms, 8 determinants), widths ((64, 16), (64, 16)): d_in counts the bias row
KFAC_LAYOUTS = {
    'lih_plain': [('single', 0, True, 3 * 8 + 2 * 4 + 1, 64, 4), ('single', 1, True, 3 * 64 + 2 * 16 + 1, 64, 4),
                  ('double', 0, True, 5, 16, 16), ('orbital', 0, False, 64, 32, 2), ('orbital', 1, False, 64, 32, 2)],
    'lih_last_bias': [('single', 0, True, 33, 64, 4), ('single', 1, True, 225, 64, 4), ('double', 0, True, 5, 16, 16),
                      ('double', 1, True, 17, 16, 16), ('orbital', 0, True, 225, 32, 2), ('orbital', 1, True, 225, 32, 2)],
}


@pytest.mark.parametrize('tag', list(H.DTYPES))
@pytest.mark.parametrize('name', list(KFAC_LAYOUTS))
def test_kfac_index_on_a_hand_written_layout(name, tag):
    """The assertions of test_gpu_kfac_step.py::test_index_map, on the CPU."""
    pm, cell, net_kw = H.param_map(name, H.DTYPES[tag])
    layout = hand_layout(KFAC_LAYOUTS[name])
    tree = numbered(H.make_tree(cell, net_kw))
    packed = pm.pack(tree, 'cpu', torch.float64)
    idx = pm.kfac_index(layout, tree)
    assert pm.kfac_index(layout, tree) is idx                       # built once per tree shape
    v = packed.index_select(0, idx['v_src'])
    off = 0
    for b in layout:
        n = b['d_in'] * b['d_out']
        got = v[off:off + n].view(b['d_in'], b['d_out']); off += n
        assert torch.equal(got, ks.block_matrix(tree, b['kind'], b['index'])), (b['kind'], b['index'])
        assert ('b' in tree[b['kind']][b['index']]) == b['has_bias']
    assert off == v.numel()
    diag = packed.index_select(0, idx['diag_src'])
    want = torch.cat([e[k].reshape(-1) for e in tree['envelope'] for k in sorted(e)])
    assert torch.equal(diag, want)
    assert all(p[0] == 'envelope' for p in idx['diag_paths'])
    total = sum(t.numel() for t in tree_leaves(tree))
    assert idx['v_tree'].numel() + idx['diag_tree'].numel() == total == sum(idx['leaf_sizes'])
    both = torch.cat([idx['v_tree'], idx['diag_tree']])
    assert torch.equal(both.sort().values, torch.arange(total))
    assert torch.equal(v, (idx['v_tree'] + 1).double())
    bad = [dict(b) for b in layout]
    bad[1]['d_in'] -= 1
    with pytest.raises(ValueError, match=r'single\[1\]: the tree holds a 225 x 64 block, the layout 224 x 64'):
        H.param_map(name, H.DTYPES[tag])[0].kfac_index(bad, tree)

"""ctypes binding of libdeepsolid_hip.so (include/deepsolid_hip.h).

There is no CPU fallback: if the shared library is missing or cannot be
loaded, every call raises.  Build it with ``python -c "import __graft_entry__
as g; g.build()"`` or ``make -C deepsolid_amd/csrc``.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DEEPSOLID_HIP_LIB: load another build of the SAME library (the sanitizer build of tools/asan_check.sh); still no fallback.
LIB_PATH = os.environ.get('DEEPSOLID_HIP_LIB') or os.path.join(_HERE, 'libdeepsolid_hip.so')

DS_MAX_LAYERS = 8
DS_MAX_SYM = 6
_PD = C.POINTER(C.c_double)


class SystemDesc(C.Structure):
    _fields_ = [
        ('dtype', C.c_int32), ('n_up', C.c_int32), ('n_dn', C.c_int32), ('n_atoms_prim', C.c_int32),
        ('prim_atoms', _PD), ('prim_a', C.c_double * 9), ('sim_a', C.c_double * 9), ('n_sym', C.c_int32),
        ('prim_AV', C.c_double * (DS_MAX_SYM * 3)), ('prim_BV', C.c_double * (DS_MAX_SYM * 3)),
        ('sim_AV', C.c_double * (DS_MAX_SYM * 3)), ('sim_BV', C.c_double * (DS_MAX_SYM * 3)),
        ('n_layers', C.c_int32), ('hidden_single', C.c_int32 * DS_MAX_LAYERS),
        ('hidden_double', C.c_int32 * DS_MAX_LAYERS), ('n_det', C.c_int32), ('distance_type', C.c_int32),
        ('envelope_type', C.c_int32), ('full_det', C.c_int32), ('use_last_layer', C.c_int32),
        ('bias_orbitals', C.c_int32), ('klist_up', _PD), ('klist_dn', _PD),
        ('n_atoms_sim', C.c_int32), ('sim_atoms', _PD), ('sim_charges', _PD), ('dist_mode', C.c_int32),
        ('n_g', C.c_int32), ('gpoints', _PD), ('gweight', _PD), ('ion_exp_re', _PD), ('ion_exp_im', _PD),
        ('ewald_alpha', C.c_double), ('ee_const', C.c_double), ('ei_const', C.c_double), ('ii_total', C.c_double),
    ]


class ParamBlock(C.Structure):
    _fields_ = [('offset', C.c_int64), ('rows', C.c_int32), ('cols', C.c_int32)]


class KfacBlock(C.Structure):
    _fields_ = [('kind', C.c_int32), ('index', C.c_int32), ('n_param_blocks', C.c_int32), ('param_blocks', C.c_int32 * 3),
                ('has_bias', C.c_int32), ('d_in', C.c_int32), ('d_out', C.c_int32), ('repeats', C.c_int32),
                ('a_offset', C.c_int64), ('g_offset', C.c_int64)]


class HfDesc(C.Structure):
    _PI = C.POINTER(C.c_int32)
    _fields_ = [
        ('a', C.c_double * 9), ('n_atoms', C.c_int32), ('atoms', _PD), ('n_shells', C.c_int32), ('shell_atom', _PI),
        ('shell_l', _PI), ('shell_nprim', _PI), ('exps', _PD), ('coefs', _PD), ('n_k', C.c_int32), ('kpts', _PD),
        ('n_images', C.c_int32), ('images', _PD), ('n_up', C.c_int32), ('n_dn', C.c_int32), ('nocc_up', _PI), ('nocc_dn', _PI),
        ('mo_up', _PD), ('mo_dn', _PD),
    ]


class EcpDesc(C.Structure):
    _PI = C.POINTER(C.c_int32)
    _fields_ = [
        ('a', C.c_double * 9), ('n_atoms', C.c_int32), ('atoms', _PD), ('atom_species', _PI), ('n_species', C.c_int32),
        ('n_l', _PI), ('r_cut_loc', _PD), ('r_cut_nl', _PD), ('term_offset', _PI), ('term_n', _PI), ('term_zeta', _PD),
        ('term_c', _PD), ('n_quad', C.c_int32),
    ]


# name -> (restype, argtypes); every symbol declared in include/deepsolid_hip.h
_VP = C.c_void_p


def _dmc_step_sig(n_lead, n_noise, n_out, ecp):
    """The three DMC step entries share their argument list: `n_lead` pointers (handles, params, the state arrays), B, steps, tau,
    tau_eff, e_trial, e_ref, e_cut, node_mode, branch_every, seed, offset, `n_noise` explicit noise arrays, (with `ecp`:
    pair_capacity,) state_valid, `n_out` output arrays, (with `ecp`: steps_done,) then ws, ws_bytes, stream."""
    step = [C.c_int64, C.c_int] + [C.c_double] * 5 + [C.c_int, C.c_int, C.c_uint64, C.c_uint64]
    return (C.c_int, [_VP] * n_lead + step + [_VP] * n_noise + ([C.c_int64] if ecp else []) + [C.c_int] + [_VP] * n_out +
            ([C.POINTER(C.c_int)] if ecp else []) + [_VP, C.c_int64, _VP])


SIGNATURES = {
    'ds_device_widths': (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'ds_system_create': (C.c_int, [C.POINTER(SystemDesc), C.POINTER(_VP)]),
    'ds_system_destroy': (None, [_VP]),
    'ds_last_error': (C.c_char_p, []),
    'ds_param_count': (C.c_int64, [_VP]),
    'ds_int8_layers': (C.c_int, [_VP]),
    'ds_pair_recompute_layers': (C.c_int, [_VP, C.c_int]),
    'ds_param_layout': (C.c_int, [_VP, C.POINTER(ParamBlock), C.c_int]),
    'ds_workspace_bytes': (C.c_int64, [_VP, C.c_int64]),
    'ds_logpsi': (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_logpsi_grad': (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_vjp_workspace_bytes': (C.c_int64, [_VP, C.c_int64]),
    'ds_logpsi_vjp': (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_pretrain_workspace_bytes': (C.c_int64, [_VP, C.c_int64]),
    'ds_pretrain_loss_vjp': (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_kfac_block_count': (C.c_int, [_VP]),
    'ds_kfac_layout': (C.c_int, [_VP, C.POINTER(KfacBlock), C.c_int]),
    'ds_kfac_workspace_bytes': (C.c_int64, [_VP, C.c_int64]),
    'ds_kfac_factors': (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_kfac_step_workspace_bytes': (C.c_int64, [_VP]),
    'ds_kfac_inverses': (C.c_int, [_VP, _VP, C.c_double, C.c_double, _VP, _VP, C.c_int64, _VP]),
    'ds_kfac_precondition': (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_kfac_inverses_sized_workspace_bytes': (C.c_int64, [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'ds_kfac_inverses_sized': (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _VP,
                                        C.c_double, C.c_double, _VP, _VP, C.c_int64, _VP]),
    'ds_jacobian_workspace_bytes': (C.c_int64, [_VP, C.c_int64]),
    'ds_logpsi_jacobian': (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, C.c_int64, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_minsr_gram_workspace_bytes': (C.c_int64, [C.c_int64, C.c_int64]),
    'ds_minsr_gram': (C.c_int, [C.c_int, _VP, C.c_int64, C.c_int64, C.c_int64, _VP, _VP, C.c_int64, _VP]),
    'ds_minsr_matvec_workspace_bytes': (C.c_int64, [C.c_int, C.c_int64, C.c_int64]),
    'ds_minsr_matvec': (C.c_int, [C.c_int, C.c_int, _VP, C.c_int64, C.c_int64, C.c_int64, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_minsr_solve_workspace_bytes': (C.c_int64, [C.c_int64, C.c_int64]),
    'ds_minsr_solve': (C.c_int, [C.c_int64, C.c_int64, C.c_double, C.c_double, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_orbitals': (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_ewald': (C.c_int, [_VP, _VP, C.c_int64, _VP, _VP]),
    'ds_local_energy': (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_enforce_pbc': (C.c_int, [_PD, C.c_int, _VP, C.c_int64, _VP, _VP, _VP]),
    'ds_observables_workspace_bytes': (C.c_int64, [C.c_int64, C.c_int]),
    'ds_observables': (C.c_int, [_PD, C.c_int, _VP, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.c_int, C.c_int, _VP, _VP,
                                 C.c_int64, _VP]),
    'ds_realspace_counts': (C.c_int, [_PD, C.POINTER(C.c_int32), _PD, _PD, C.c_double, C.c_int, C.c_int, _VP, C.c_int64, C.c_int64,
                                      C.c_int64, _VP, _VP, _VP]),
    'ds_mh_propose': (C.c_int, [_VP, _VP, _VP, C.c_double, C.c_int64, _VP, _VP]),
    'ds_mh_accept': (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP, _VP]),
    'ds_mh_propose_ex': (C.c_int, [_VP, C.c_int, _VP, _VP, C.c_double, _VP, C.c_int, C.c_int64, _VP, _VP, _VP]),
    'ds_mh_accept_ex': (C.c_int, [_VP, C.c_int, _VP, _VP, _VP, _VP, _VP, _VP, C.c_double, _VP, _VP, C.c_int, C.c_int64, _VP, _VP, _VP]),
    'ds_mcmc_workspace_bytes': (C.c_int64, [_VP, C.c_int64]),
    'ds_mcmc_step': (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, C.c_int, C.c_double, C.c_uint64, C.c_uint64, _VP, _VP, C.c_int, _VP, _VP,
                              C.c_int64, _VP]),
    'ds_mcmc_step_one_electron': (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_uint64, C.c_uint64, _VP, _VP,
                                           C.c_int, _VP, _VP, C.c_int64, _VP]),
    'ds_mcmc_step_importance': (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, C.c_int, C.c_double, C.c_uint64, C.c_uint64, _VP, _VP, C.c_int,
                                         _VP, _VP, C.c_int64, _VP]),
    'ds_mcmc_step_asymmetric': (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, C.c_int, C.c_double, _VP, C.c_int, C.c_uint64, C.c_uint64, _VP, _VP,
                                         C.c_int, _VP, _VP, C.c_int64, _VP]),
    'ds_one_body_workspace_bytes': (C.c_int64, [_VP, C.c_int64, C.c_int]),
    'ds_one_body_ratios': (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int, C.c_int, C.c_uint64, C.c_uint64, _VP, _VP, C.c_int, _VP, _VP, _VP,
                                     _VP, _VP, C.c_int64, _VP]),
    'ds_spin_exchange_workspace_bytes': (C.c_int64, [_VP, C.c_int64, C.c_int]),
    'ds_spin_exchange_ratios': (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int, C.c_int, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_ion_forces_workspace_bytes': (C.c_int64, [_VP, C.c_int64]),
    'ds_ion_forces': (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_double, _VP, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_stress_workspace_bytes': (C.c_int64, [_VP, C.c_int64]),
    'ds_stress': (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_ion_vjp_workspace_bytes': (C.c_int64, [_VP, C.c_int64]),
    'ds_logpsi_ion_vjp': (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_ecp_create': (C.c_int, [C.POINTER(EcpDesc), C.POINTER(_VP)]),
    'ds_ecp_destroy': (None, [_VP]),
    'ds_ecp_workspace_bytes': (C.c_int64, [_VP, _VP, C.c_int64, C.c_int64]),
    'ds_ecp_energy': (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, C.c_uint64, C.c_uint64, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP,
                               C.c_int64, _VP]),
    'ds_ecp_forces_workspace_bytes': (C.c_int64, [_VP, _VP, C.c_int64, C.c_int64]),
    'ds_ecp_forces': (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, C.c_uint64, C.c_uint64, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP,
                               _VP, C.c_int64, _VP]),
    'ds_dmc_workspace_bytes': (C.c_int64, [_VP, C.c_int64]),
    'ds_dmc_step': _dmc_step_sig(8, 3, 2, ecp=False),
    'ds_dmc_ecp_workspace_bytes': (C.c_int64, [_VP, _VP, C.c_int64, C.c_int64]),
    'ds_dmc_step_ecp': _dmc_step_sig(10, 4, 4, ecp=True),
    'ds_dmc_tmove_workspace_bytes': (C.c_int64, [_VP, _VP, C.c_int64, C.c_int64]),
    'ds_dmc_step_tmove': _dmc_step_sig(10, 5, 6, ecp=True),
    'ds_dmc_noise': (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_uint64, C.c_uint64, _VP, _VP, _VP, _VP]),
    'ds_dmc_branch_workspace_bytes':(C.c_int64, [C.c_int, C.c_int, C.c_int64]),
    'ds_dmc_branch': (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_double, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_dmc_ancestry_workspace_bytes': (C.c_int64, [C.c_int64, C.c_int]),
    'ds_dmc_ancestry': (C.c_int, [C.c_int64, C.c_int, _VP, C.c_int, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_realspace_counts_w': (C.c_int, [_PD, C.POINTER(C.c_int32), _PD, _PD, C.c_double, C.c_int, C.c_int, _VP, C.c_int64, C.c_int64,
                                        C.c_int64, _VP, _VP, C.c_int64, _VP, _VP, C.c_double, _VP, _VP, _VP]),
    'ds_dmc_fw_sums_workspace_bytes': (C.c_int64, [C.c_int64, C.c_int]),
    'ds_dmc_fw_sums': (C.c_int, [C.c_int64, C.c_int, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP]),
    'ds_philox_host': (None,[C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint32)]),
    'ds_energy_stats': (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP]),
    'ds_debug_stage': (C.c_int64, [_VP, _VP, _VP, C.c_int64, C.c_char_p, _VP, C.c_int64, _VP, C.c_int64, _VP]),
    'ds_profile_enable': (C.c_int, [_VP, C.c_int]),
    'ds_profile_read': (C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'ds_profile_read_clock': (C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'ds_debug_timeline': (C.c_int, [_VP, C.POINTER(C.c_uint64), C.c_int]),
    'ds_calib_copy': (C.c_int, [_VP, _VP, C.c_int64, _VP]),
    'ds_mfma_f64_peak': (C.c_int64, [C.c_int64, C.c_int, C.c_int, _VP, _VP]),
    'ds_hf_create': (C.c_int, [C.POINTER(HfDesc), C.POINTER(_VP)]),
    'ds_hf_destroy': (None, [_VP]),
    'ds_hf_orbitals': (C.c_int, [_VP, C.c_int, _VP, C.c_int64, _VP, _VP, _VP]),
    'ds_hf_orbitals_at': (C.c_int, [_VP, C.c_int, C.c_int, _VP, C.c_int64, _VP, _VP]),
    'ds_obdm_workspace_bytes': (C.c_int64, [_VP, C.c_int64, C.c_int]),
    'ds_obdm_accumulate': (C.c_int, [_VP, C.c_int, _VP, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                     C.c_int64, _VP]),
}

PROF_KINDS = ('features', 'm2_expand', 'two_layer', 'single_first', 'single_hidden', 'orbital', 'det_inverse',
              'det_trace', 'combine', 'ewald', 'shared_term', 'single_lr', 'ion_vjp')

_lib = None


def load():
    """Load the HIP library (once).  Raises RuntimeError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f'{LIB_PATH} is missing: the HIP extension is not built and deepsolid_amd has no CPU '
            'fallback.  Run `make -C deepsolid_amd/csrc` (hipcc, --offload-arch=gfx950).')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().ds_last_error()
        raise RuntimeError(f'{what} failed: {msg.decode() if msg else rc}')

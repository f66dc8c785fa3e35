#!/usr/bin/env python3
"""End-to-end example on one MI355X: variational Monte Carlo of the 4-electron LiH cell with the reference's default
network -- a few Adam (or KFAC, or SPRING) iterations (train.py / process.py), then an energy evaluation of the result
(process.py `optimizer='none'`).  Synthetic start (random parameters, uniform walkers): the numbers are not physics,
the point is the call sequence.  usage: python examples/vmc_lih.py [iterations] [batch] [--pretrain N] [--optimizer adam|kfac|spring]   (N iterations of orbital-matching pretraining against
the plane waves of the network's own k list first, process.py:148-177; --optimizer kfac: the reference's default optimizer,
process.py:209-228, with the learning-rate schedule of base_config.py:46-51; --optimizer spring: SPRING on the per-walker Jacobian,
deepsolid_amd.spring, with the same schedule;
--hf FILE.npz: pretrain against the Hartree-Fock orbitals dumped into FILE.npz (deepsolid_amd.hf.GaussianOrbitals, INTEGRATION.md:
a calculation of THIS 4-electron cell) instead of plane waves, the network taking the file's k list; --pretrain-method net|hf:
move the pretraining walkers on the network's density or on the Hartree-Fock density, process.py:148,164; hf needs --hf;
--density G: accumulate the spin-resolved electron density on a G^3 grid of the primitive cell over the evaluation;
--pair-correlation BINS: the spin-resolved g(r) on BINS radial bins up to the Wigner-Seitz radius -- both through
deepsolid_amd.estimator.RealSpaceAccumulator, written to realspace.npz in the working directory;
--momentum SHELLS: the spin-resolved momentum distribution n(k) on the (2 SHELLS + 1)^3 Bloch-allowed k points around the twist,
through deepsolid_amd.estimator.MomentumDistribution, written to momentum.npz;
--obdm: with --hf, the spin-resolved one-body density matrix in the basis of the file's orbitals and its natural occupation numbers,
through deepsolid_amd.estimator.OneBodyDensityMatrix, written to obdm.npz;
--spin-squared [PAIRS]: the total spin <S^2> from PAIRS spin-exchange ratios per walker and evaluation step (default: all
n_up n_dn pairs), through deepsolid_amd.estimator.SpinSquared, written to spin_squared.npz;
--forces: the forces on the two ions over the evaluation, through deepsolid_amd.estimator.IonForces, written to forces.npz: the
Hellmann-Feynman force of the Ewald energy and the zero-variance force of Assaraf and Caffarel with the Wigner-Seitz radius as its
cutoff; --forces-cutoff X: the same with the cutoff X in bohr (at most the Wigner-Seitz radius).  The Pulay term is NOT evaluated,
so both are the force only for an exact wave function (bias first order in its error); all-electron only: not with --ecp;
--forces-total: the TOTAL force per atom of the primitive cell (zero-variance force + Pulay term), through
deepsolid_amd.estimator.PrimitiveForces, written to forces_total.npz; one block per evaluation step, errors by reblocking the block
series; honours --forces-cutoff; all-electron only: not with --ecp;
--forces-ecp: with --ecp, the forces on the two ions of the pseudopotential cell over the evaluation, through
deepsolid_amd.estimator.PseudopotentialForces, written to forces_ecp.npz: pp = minus the derivative of E_loc + E_nl in the ion
position, total = pp + the Hellmann-Feynman force of the Ewald energy with Z_eff.  Hellmann-Feynman part only (no Pulay term: bias
first order in the error of psi), the delta term of the cutoffs is left out, and it costs one forward-Laplacian chain evaluation
per quadrature configuration;
--stress: the stress tensor and the pressure of the cell over the evaluation, through deepsolid_amd.estimator.StressTensor, written to
stress.npz: the integrated-by-parts kinetic tensor plus the strain derivative of the Ewald sums over the volume, naive errors.  The
change of psi with the cell at fixed parameters is NOT evaluated, so it is the stress only for an exact wave function; all-electron
only: not with --ecp;
--stress-total: the same with the wave-function term (StressTensor(wavefunction_term=True): twelve strained handles, twelve more
forwards per evaluation step, one block per step, errors by reblocking), written to stress_total.npz;
--ecp FILE.npz: add the semi-local pseudopotential saved in FILE.npz (deepsolid_amd.pseudopotential.SemiLocalECP.save, built for
THIS cell) to the local energy of training and evaluation: the rows then carry its batch mean E_loc + E_nl.  The
cell of this example is all-electron, so with a real potential the numbers mean nothing: the point is the call sequence);
--dmc BLOCKS [--dmc-tau TAU]: after the evaluation, BLOCKS blocks of 20 steps of fixed-phase diffusion Monte Carlo at time step TAU
(default 0.01) from the evaluation's walkers, through deepsolid_amd.inference.run_dmc; with --ecp in the locality
approximation, the rows then carrying the mixed estimate of E_loc + E_nl;
--dmc-pure LAG[,LAG...]: with --dmc, pure estimators by forward walking at these lags, counted in blocks (deepsolid_amd.dmc.ForwardWalking,
DESIGN.md section 19.3): for every lag the pure potential, kinetic and total energy and the largest density difference to lag 0
(the properly weighted mixed estimate, which is always tracked);
--tmoves: with --ecp and --dmc, Casula's T-moves in place of the locality approximation: the energy is then
an upper bound, and the rows carry the T-moves per walker and step)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from deepsolid_amd import inference, network, systems

n_pre = 0
if '--pretrain' in sys.argv:
    i = sys.argv.index('--pretrain')
    n_pre = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
optimizer = 'adam'
if '--optimizer' in sys.argv:
    i = sys.argv.index('--optimizer')
    optimizer = sys.argv[i + 1]
    del sys.argv[i:i + 2]
scf_approx, pretrain_method = None, 'net'
if '--hf' in sys.argv:
    from deepsolid_amd import hf
    i = sys.argv.index('--hf')
    scf_approx = hf.GaussianOrbitals.load(sys.argv[i + 1])
    del sys.argv[i:i + 2]
if '--pretrain-method' in sys.argv:
    i = sys.argv.index('--pretrain-method')
    pretrain_method = sys.argv[i + 1]
    del sys.argv[i:i + 2]
density_grid = pair_bins = None
if '--density' in sys.argv:
    i = sys.argv.index('--density')
    density_grid = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
if '--pair-correlation' in sys.argv:
    i = sys.argv.index('--pair-correlation')
    pair_bins = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
momentum_shells = None
if '--momentum' in sys.argv:
    i = sys.argv.index('--momentum')
    momentum_shells = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
obdm = '--obdm' in sys.argv
if obdm:
    sys.argv.remove('--obdm')
    if scf_approx is None:
        sys.exit('--obdm needs --hf FILE.npz: the orbitals of the file are the basis of the density matrix')
spin_squared, spin_pairs = False, None
if '--spin-squared' in sys.argv:
    i = sys.argv.index('--spin-squared')
    spin_squared = True
    if i + 1 < len(sys.argv) and sys.argv[i + 1].isdigit():      # (the option takes a number that follows it: give iterations / batch first)
        spin_pairs = int(sys.argv[i + 1])
        del sys.argv[i + 1]
    del sys.argv[i]
forces_total = '--forces-total' in sys.argv
if forces_total:
    sys.argv.remove('--forces-total')
forces, force_cutoff = False, None
if '--forces-cutoff' in sys.argv:
    i = sys.argv.index('--forces-cutoff')
    forces, force_cutoff = not forces_total, float(sys.argv[i + 1])
    del sys.argv[i:i + 2]
if '--forces' in sys.argv:
    forces = True
    sys.argv.remove('--forces')
forces_ecp = '--forces-ecp' in sys.argv
if forces_ecp:
    sys.argv.remove('--forces-ecp')
stress_total = '--stress-total' in sys.argv
if stress_total:
    sys.argv.remove('--stress-total')
stress = '--stress' in sys.argv
if stress:
    sys.argv.remove('--stress')
dmc_blocks, dmc_tau = 0, 0.01
if '--dmc-tau' in sys.argv:
    i = sys.argv.index('--dmc-tau')
    dmc_tau = float(sys.argv[i + 1])
    del sys.argv[i:i + 2]
dmc_pure = None
if '--dmc-pure' in sys.argv:
    i = sys.argv.index('--dmc-pure')
    dmc_pure = tuple(sorted({0} | {int(v) for v in sys.argv[i + 1].split(',')}))
    del sys.argv[i:i + 2]
if '--dmc' in sys.argv:
    i = sys.argv.index('--dmc')
    dmc_blocks = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
tmoves = '--tmoves' in sys.argv
if tmoves:
    sys.argv.remove('--tmoves')
ecp_file = None
if '--ecp' in sys.argv:
    i = sys.argv.index('--ecp')
    ecp_file = sys.argv[i + 1]
    del sys.argv[i:i + 2]
if (forces or forces_total) and ecp_file is not None:
    sys.exit('--forces / --forces-total is all-electron only: the force terms of a pseudopotential are not implemented')
if forces_ecp and ecp_file is None:
    sys.exit('--forces-ecp needs --ecp FILE.npz')
if (stress or stress_total) and ecp_file is not None:
    sys.exit('--stress / --stress-total is all-electron only: the strain derivative of a pseudopotential is not implemented')
if dmc_pure is not None and dmc_blocks <= 0:
    sys.exit('--dmc-pure needs --dmc BLOCKS')
if tmoves and (ecp_file is None or dmc_blocks <= 0):
    sys.exit('--tmoves needs --ecp FILE.npz and --dmc BLOCKS')
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
batch = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
cell, klist = systems.build('lih')
if scf_approx is not None:
    if scf_approx.nelec != tuple(cell.nelec):
        sys.exit(f'--hf: the file holds nelec = {scf_approx.nelec}, this cell has {tuple(cell.nelec)}')
    klist = scf_approx.klist
ecp = None
if ecp_file is not None:
    from deepsolid_amd.pseudopotential import SemiLocalECP
    ecp = SemiLocalECP.load(ecp_file, cell)
kw = dict(systems.DETNET_DEFAULTS)
logdet = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **kw)
slogdet = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_slogdet', **kw)
params = logdet.init(0)
data = torch.as_tensor(systems.synthetic_walkers(cell, batch), device='cuda')
data, params, state, width, rows = inference.run_training(slogdet, logdet, params, data, cell, iterations=iters, burn_in=20,
                                                          learning_rate=2e-3 if optimizer == 'adam' else None, move_width=0.1,
                                                          pretrain_iterations=n_pre, optimizer=optimizer, scf_approx=scf_approx,
                                                          pretrain_method=pretrain_method, pseudopotential=ecp)
print('training:   E[0] = %.4f  ->  E[%d] = %.4f Ha   (pmove %.2f)' % (rows[0]['energy'], iters - 1, rows[-1]['energy'], rows[-1]['pmove']))
accumulators = ()
if density_grid is not None or pair_bins is not None:
    from deepsolid_amd import estimator
    accumulators = (estimator.RealSpaceAccumulator(cell, density_grid=density_grid, pair_bins=pair_bins),)
if momentum_shells is not None:
    from deepsolid_amd import estimator
    accumulators += (estimator.MomentumDistribution(logdet, params, shells=momentum_shells),)
momentum_acc = accumulators[-1] if momentum_shells is not None else None
obdm_acc = None
if obdm:
    from deepsolid_amd import estimator
    obdm_acc = estimator.OneBodyDensityMatrix(logdet, params, scf_approx)
    accumulators += (obdm_acc,)
spin_acc = None
if spin_squared:
    from deepsolid_amd import estimator
    spin_acc = estimator.SpinSquared(logdet, params, pairs_per_walker=spin_pairs)
    accumulators += (spin_acc,)
force_acc = None
if forces:
    from deepsolid_amd import estimator
    force_acc = estimator.IonForces(logdet, params, cutoff=force_cutoff)
    accumulators += (force_acc,)
total_acc = None
if forces_total:
    from deepsolid_amd import estimator
    total_acc = estimator.PrimitiveForces(logdet, params, cutoff=force_cutoff)
    accumulators += (total_acc,)
ecp_force_acc = None
if forces_ecp:
    from deepsolid_amd import estimator
    ecp_force_acc = estimator.PseudopotentialForces(logdet, params, ecp)
    accumulators += (ecp_force_acc,)
stress_acc = None
if stress:
    from deepsolid_amd import estimator
    stress_acc = estimator.StressTensor(logdet, params)
    accumulators += (stress_acc,)
stress_total_acc = None
if stress_total:
    from deepsolid_amd import estimator
    stress_total_acc = estimator.StressTensor(logdet, params, wavefunction_term=True)
    accumulators += (stress_total_acc,)
data, width, rows = inference.run_inference(slogdet, logdet, params, data, cell, iterations=10, burn_in=10, move_width=width,
                                            accumulators=accumulators, pseudopotential=ecp)
if ecp is not None:
    print('pseudopotential: <E_loc + E_nl> = %.4f Ha (N_q = %d)' % (sum(r['pseudopotential'].real for r in rows) / len(rows), ecp.n_quad))
print('evaluation: E = %.4f +- %.4f Ha over 10 x %d walkers' % (sum(r['energy'] for r in rows) / len(rows),
                                                                (sum(r['variance'] for r in rows) / len(rows) / (10 * batch)) ** 0.5, batch))
for acc in accumulators:
    if acc is spin_acc:
        acc.save('spin_squared.npz', results=True)
        s2 = acc.spin_squared()
        print('<S^2>:      %.4f +- %.4f (naive error over %d walkers, %d left out; %d of %d pairs per walker; S_z (S_z + 1) = %.2f)'
              % (s2['value'], s2['error'], s2['n_walkers'], s2['n_bad'], acc.pairs_per_walker, acc.n_pairs_total, s2['sz'] * (s2['sz'] + 1)))
        continue
    if acc is force_acc:
        acc.save('forces.npz', results=True)
        f = acc.forces()
        print('forces:     cutoff %.4f Bohr, naive errors over %d walkers (%d left out); no Pulay term: exact only for an exact psi'
              % (f['cutoff'], f['n_walkers'], f['n_bad']))
        for a in range(len(f['atoms'])):
            print('            %-2s HF (%9.4f %9.4f %9.4f) +- (%.4f %.4f %.4f)   ZV (%9.4f %9.4f %9.4f) +- (%.4f %.4f %.4f) Ha/Bohr'
                  % ((cell.atom_symbol(a),) + tuple(f['hf'][a]) + tuple(f['hf_error'][a]) + tuple(f['zv'][a]) + tuple(f['zv_error'][a])))
        continue
    if acc is total_acc:
        acc.save('forces_total.npz', results=True)
        f = acc.forces()
        print('total force per primitive atom and simulation cell: cutoff %.4f Bohr, %d blocks, %d walkers (%d left out), reblocked errors'
              % (f['cutoff'], f['n_blocks'], f['n_walkers'], f['n_bad']))
        prim = cell.original_cell
        for a in range(len(f['atoms'])):
            print('            %-2s total (%9.4f %9.4f %9.4f) +- (%.4f %.4f %.4f)   ZV (%9.4f %9.4f %9.4f)   Pulay (%9.4f %9.4f %9.4f) Ha/Bohr'
                  % ((prim.atom_symbol(a),) + tuple(f['total'][a]) + tuple(f['total_error'][a]) + tuple(f['zv'][a]) + tuple(f['pulay'][a])))
        continue
    if acc is ecp_force_acc:
        acc.save('forces_ecp.npz', results=True)
        f = acc.forces()
        print('pseudopotential forces: naive errors over %d walkers (%d left out); Hellmann-Feynman part only, no cutoff delta term'
              % (f['n_walkers'], f['n_bad']))
        for a in range(len(f['atoms'])):
            print('            %-2s pp (%9.4f %9.4f %9.4f) +- (%.4f %.4f %.4f)   total (%9.4f %9.4f %9.4f) +- (%.4f %.4f %.4f) Ha/Bohr'
                  % ((cell.atom_symbol(a),) + tuple(f['pp'][a]) + tuple(f['pp_error'][a]) + tuple(f['total'][a]) + tuple(f['total_error'][a])))
        continue
    if acc is stress_acc:
        acc.save('stress.npz', results=True)
        t = acc.stress()
        print('stress:     V = %.3f Bohr^3, naive errors over %d walkers (%d left out); no wave-function term: exact only for an exact psi'
              % (t['volume'], t['n_walkers'], t['n_bad']))
        for a in range(3):
            print('            (%10.6f %10.6f %10.6f) +- (%.6f %.6f %.6f) Ha/Bohr^3' % (tuple(t['sigma'][a]) + tuple(t['sigma_error'][a])))
        print('            P = %.6f +- %.6f Ha/Bohr^3 = %.2f +- %.2f GPa' % (t['pressure'], t['pressure_error'], t['pressure_gpa'],
                                                                           t['pressure_gpa_error']))
        continue
    if acc is stress_total_acc:
        acc.save('stress_total.npz', results=True)
        t = acc.stress()
        print('total stress: %d blocks, %d walkers (%d left out), reblocked errors; with the wave-function term' % (t['n_blocks'], t['n_walkers'], t['n_bad']))
        for a in range(3):
            print('            (%10.6f %10.6f %10.6f) +- (%.6f %.6f %.6f) Ha/Bohr^3' % (tuple(t['sigma_total'][a]) + tuple(t['sigma_total_error'][a])))
        print('            P = %.6f +- %.6f Ha/Bohr^3 = %.2f GPa' % (t['pressure_total'], t['pressure_total_error'], t['pressure_total_gpa']))
        continue
    if acc is obdm_acc:
        acc.save('obdm.npz', results=True)
        print('1-RDM:      %d / %d basis functions, %d / %d samples (%d / %d left out); no error bars'
              % (acc.norb + tuple(acc.samples) + (int(acc.n_bad[0]), int(acc.n_bad[1]))))
        for sp, name in enumerate(('up', 'down')):
            if acc.norb[sp] and acc.nelec[sp]:
                occ = acc.natural_orbitals(sp)[0]
                print('            natural occupations %-4s (sampled overlap): %s   sum = %.4f of %d electrons'
                      % (name, ' '.join('%.4f' % v for v in occ), occ.sum(), acc.nelec[sp]))
        continue
    if acc is momentum_acc:
        acc.save('momentum.npz', results=True)
        nk = acc.momentum_distribution().real
        print('n(k):       %d k points, %d / %d samples (%d / %d left out); n_up(k_t) = %.4f, n_down(k_t) = %.4f, sums over k = %.4f / %.4f'
              % (nk.shape[1], acc.samples[0], acc.samples[1], int(acc.n_bad[0]), int(acc.n_bad[1]), nk[0, 0], nk[1, 0],
                 nk[0].sum(), nk[1].sum()))
        continue
    acc.save('realspace.npz', results=True)
    if density_grid is not None:
        rho = acc.density()
        dv = abs(float(np.linalg.det(acc.fold))) / rho[0].size
        print('density:    %d^3 grid, %d walkers, up / down electrons per primitive cell = %.6f / %.6f, max %.4f e/Bohr^3'
              % (density_grid, acc.n_walkers, rho[0].sum() * dv, rho[1].sum() * dv, rho.max()))
    if pair_bins is not None:
        r, g = acc.pair_correlation()
        print('g(r):       %d bins to r_max = %.3f Bohr; last bin up-up %.3f, up-down %.3f, down-down %.3f'
              % (pair_bins, acc.r_max, g[0, -1], g[1, -1], g[2, -1]))
if dmc_blocks > 0:
    from deepsolid_amd import dmc
    tracker = None if dmc_pure is None else dmc.ForwardWalking(cell, lags=dmc_pure, density_grid=16, pair_bins=32)
    state, dmc_rows, info = inference.run_dmc(slogdet, logdet, params, data, cell, blocks=dmc_blocks, steps_per_block=20, tau=dmc_tau,
                                              move_width=width, burn_in=10, pseudopotential=ecp, tmoves=tmoves,
                                              forward_walking=tracker)
    e, err, length = dmc.reblock([r['energy'] for r in dmc_rows[len(dmc_rows) // 4:]])
    print('VMC:        E = %.4f +- %.4f Ha' % (info['vmc_energy'], info['vmc_error']))
    print('DMC:        E = %.4f +- %.4f Ha (tau = %g, %d blocks of 20 steps, the first quarter left out; acceptance %.4f, '
          'tau_eff %.5f, %d walkers killed)' % (e, err, dmc_tau, dmc_blocks, sum(r['acceptance'] for r in dmc_rows) / len(dmc_rows),
                                                dmc_rows[-1]['tau_eff'], sum(r['killed'] for r in dmc_rows)))
    if ecp is not None:
        print('            %s: mixed <E_loc + E_nl> = %.4f Ha'
              % ('T-moves' if tmoves else 'locality approximation', sum(r['pseudopotential'].real for r in dmc_rows) / len(dmc_rows)))
    if tmoves:
        print('            %.4f T-moves per walker and step' % (sum(r['tmoves'] for r in dmc_rows) / len(dmc_rows)))
    if tracker is not None:
        skip = dmc_blocks // 4
        for lag in dmc_pure:
            (e, err, _), (v, _, _), (k, _, _) = (tracker.scalar(n, lag, skip=skip) for n in ('energy', 'potential', 'kinetic'))
            diff = abs(tracker.density(lag) - tracker.density(0)).max()
            print('pure, lag %2d blocks: V = %.4f  T = %.4f  E = %.4f +- %.4f Ha per simulation cell; largest density difference to '
                  'lag 0: %.3e e/Bohr^3' % (lag, v, k, e, err, diff))

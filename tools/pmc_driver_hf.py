#!/usr/bin/env python3
"""Workload for a counter pass over the Hartree-Fock orbital kernel: tools/hf_bench.py's diamond case (96 e-, 28 AOs, n_k = 8,
B = 1024), the orbital kernel alone, 1 warm-up + 3 launches.  PMC_HF_CASE=bcc_li selects the other case."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hf_bench

sys.argv = [sys.argv[0], '--case', os.environ.get('PMC_HF_CASE', 'diamond'), '--only-hf', '--warmup', '1', '--calls', '3']
hf_bench.main()

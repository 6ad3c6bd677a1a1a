"""kernel launches of EnsembleBatch runs at B = 16 and 1 024 (5 000 steps: two chunks of <= 4 096 steps)"""
import sys
import numpy as np
sys.path.insert(0, ".")
from emcee_amd import EnsembleBatch, targets
for B in (16, 1024):
    bt = EnsembleBatch(B, 32, 5, targets.IsoGaussian(), seeds=list(range(B)))
    bt.run_mcmc(np.random.RandomState(0).randn(B, 32, 5), 5000, store=False)
    print(B, bt.launch_info(), flush=True)
    bt.close()

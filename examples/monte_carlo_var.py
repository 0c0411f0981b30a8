# Monte Carlo value-at-risk in plain numpy: the lower percentiles, the median
# and the most populated histogram bin of simulated standard-normal returns.
# With numpy_offload=True the draw lives on the sandbox's MI355X (2 000 000 is
# above the offload threshold); np.percentile and np.median are radix selects
# of a few ranks (no sort) and np.histogram counts in LDS, all on the GPU
# (ops/numpy_offload.py, csrc/kernels/stats.hip).  Only the few results come
# back; without the offload it is plain CPU numpy.

import numpy as np

n = 2_000_000
np.random.seed(7)
r = np.random.normal(0.0, 1.0, n)
var_1, var_5 = np.percentile(r, [1, 5])
print("VaR 1%:", var_1)
print("VaR 5%:", var_5)
print("Median:", np.median(r))
counts, edges = np.histogram(r, bins=50)
mode = max(range(len(counts)), key=lambda i: counts[i])
print("Mode bin:", edges[mode], edges[mode + 1], "count", counts[mode])

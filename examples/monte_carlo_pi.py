# Monte Carlo estimate of pi in plain numpy: the fraction of uniform points of
# the unit square that fall inside the quarter circle.  With
# numpy_offload=True the draws live on the sandbox's MI355X (4 000 000 is
# above the offload threshold), the comparison returns a device mask,
# numpy.sum of it is one fused compare-count pass, and x[inside] is a stream
# compaction on the GPU (ops/numpy_offload.py); without the offload it is
# plain CPU numpy.

import numpy as np

n = 4_000_000
x = np.random.rand(n)
y = np.random.rand(n)
inside = x**2 + y**2 <= 1.0
pi = 4 * np.sum(inside) / n
print("Pi:", pi)
print("Mean x inside:", x[inside].mean())

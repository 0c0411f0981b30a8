# Aggregate insurance loss in plain numpy: every policy has a gamma frailty
# (its own claim rate), an exponential waiting time to its first claim at that
# rate and a lognormal claim size; a policy pays if the claim falls inside the
# period.  With numpy_offload=True the three draws are made on the sandbox's
# MI355X (2 000 000 is above the offload threshold: exponential and lognormal
# are one fused Philox-to-transform kernel each, gamma a Marsaglia-Tsang
# rejection kernel, csrc/kernels/random.hip) and the division, the comparison
# mask, the selection by it, the means, the percentile and the maximum all run
# there too.  Only the printed scalars come back; without the offload it is
# plain CPU numpy.

import numpy as np

n = 2_000_000
np.random.seed(11)
frailty = np.random.gamma(2.0, 0.5, n)            # mean 1: the policy's claim rate
severity = np.random.lognormal(0.0, 1.0, n)       # the size of its claim
wait = np.random.exponential(1.0, n) / frailty    # time to the first claim at that rate
claimed = wait < 1.0                              # inside the period of length 1
paid = severity[claimed]
frequency = np.mean(claimed)
print("Claim frequency:", frequency)
print("Mean paid claim:", paid.mean())
print("Loss per policy:", frequency * paid.mean())
print("99% paid claim:", np.percentile(paid, 99))
print("Largest claim:", np.max(paid))

# Dice, claim counts and coin flips: the integer-valued draws of beekern, made
# and summarised on the sandbox's MI355X (csrc/kernels/integer.hip).  The dice
# are uniform int64 draws by Lemire's multiply-shift; their sum, the comparison
# with 7 and the mean of the mask are int64 and mask kernels.  Every policy
# then draws a Poisson claim count at the mean rate of a gamma frailty, and a
# player tallies the heads of ten fair coins (numpy's multiplication and
# inversion methods on Philox substreams).  Only the printed scalars come back
# to the host; nothing falls back to host numpy.  (A device array's == is
# Python's identity, so the comparison is spelled np.equal.)

import numpy as np

import beekern as bk

n = 2_000_000
rng = bk.random.default_rng(7)

total = rng.integers(1, 7, n) + rng.integers(1, 7, n)
print("P(total is 7):", np.mean(np.equal(total, 7)))
print("Mean total:", np.mean(total))
print("Largest total:", np.max(total))

rate = float(np.mean(rng.gamma(2.0, 0.5, n)))      # the frailty's mean rate, 1 up to sampling error
claims = rng.poisson(rate, n)
print("Claim rate:", rate)
print("Mean claims per policy:", np.mean(claims))
print("Share with two or more claims:", np.mean(claims >= 2))

heads = rng.binomial(10, 0.5, n)
print("Mean heads in ten flips:", np.mean(heads))
print("Share with eight or more heads:", np.mean(heads >= 8))
print("Total heads:", np.sum(heads))

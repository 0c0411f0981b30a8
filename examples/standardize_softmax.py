# Tables in plain numpy: standardise the columns of a samples x features matrix,
# take a softmax of every row, and check the correlation matrix's diagonal.
# With numpy_offload=True the table lives on the sandbox's MI355X (6 400 000
# elements are above the offload threshold): X - X.mean(axis=0) and the two
# divisions broadcast a vector along one axis in one pass, std / max / sum along
# an axis are one reduction each (keepdims is a reshape), and Z.T @ Z is the f64
# GEMM reading the transposed view in place (ops/numpy_offload.py,
# csrc/kernels/axis.hip).  Only the printed numbers and the 32 x 32 matrix come
# back; without the offload it is plain CPU numpy.

import numpy as np

np.random.seed(11)
X = np.random.normal(5.0, 3.0, (200000, 32))

Z = (X - X.mean(axis=0)) / X.std(axis=0)
col_std = Z.std(axis=0)
print("Largest |column mean|:", np.abs(Z.mean(axis=0)).max())
print("Column std range:", col_std.min(), col_std.max())

E = np.exp(Z - Z.max(axis=1, keepdims=True))
P = E / E.sum(axis=1, keepdims=True)
row_sums = P.sum(axis=1)
print("Softmax row sums:", row_sums.min(), row_sums.max())

C = (Z.T @ Z) / Z.shape[0]
diag = np.diag(np.asarray(C))
print("Correlation diagonal:", diag.min(), diag.max())

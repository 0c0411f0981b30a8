# The largest claims of a simulated book, ranked on the sandbox's MI355X
# (csrc/kernels/sort.hip).  Two million lognormal claim sizes are ordered by a
# stable radix argsort; the ten largest and the median are gathered from that
# order with x[idx], the worst scenario is found by argmax, and a second array
# (each claim's region) is reordered by the first one's order.  Only the printed
# scalars come back to the host; nothing falls back to host numpy.

import beekern as bk

n = 2_000_000
rng = bk.random.default_rng(11)
severity = rng.lognormal(8.0, 1.5, n)
region = rng.integers(0, 50, n)


def report(out, top, top_at, worst_at, worst, top_regions, median):
    out("Ten largest claims:", " ".join(f"{v:.2f}" for v in top))
    out("Their scenario numbers:", " ".join(str(i) for i in top_at))
    out("Worst scenario:", worst_at, f"{worst:.2f}")
    out("Regions of the ten largest:", " ".join(str(r) for r in top_regions))
    out("Median claim:", f"{median:.4f}")


order = bk.argsort(severity)                      # int64, ascending and stable, on the device
from_the_top = [n - 1 - k for k in range(10)]
largest_at = order[from_the_top]                  # the scenarios of the ten largest claims, largest first
largest = severity[largest_at]
worst_at = bk.argmax(severity)
region_by_size = region[order]                    # another array in the first one's order
ranked = severity[order]                          # what bk.sort(severity) holds

report(print, largest.numpy().tolist(), largest_at.numpy().tolist(), int(worst_at), float(severity[[int(worst_at)]].numpy()[0]),
       region_by_size[from_the_top].numpy().tolist(), float(ranked[[n // 2]].numpy()[0]))

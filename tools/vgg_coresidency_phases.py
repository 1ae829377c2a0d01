"""Phases of ONE full training step and the time of the 16x16x128 VGG19 conv tile in it, from a rocprofv3 kernel trace (steps delimited by k_adam, as tools/critical_path.py):
    forward end  = start of the first k_time_chunk (the loss call gathers the first chunk's frames: the model's forward pass and the L1 terms are behind it)
    replay start = start of the first k_map<FBnBwdApply...> (the tape replay's first BatchNorm backward); replay length = step end - replay start
and the summed duration / launches of k_conv_hx<.., 16, 16, 128, 4, 2, ..> (8 waves) and <.., 16, 16, 128, 4, 1, ..> (co-resident instance) and of k_wgrad_hx.
    python tools/vgg_coresidency_phases.py <results.db>"""
import re
import sqlite3
import sys

c = sqlite3.connect(sys.argv[1])
rows = c.execute("select name,start,end from kernels order by start").fetchall()
ad = [i for i, r in enumerate(rows) if "k_adam" in r[0]]
seg = rows[ad[1] + 1:ad[2] + 1] if len(ad) >= 3 else rows
t0, t1 = seg[0][1], seg[-1][2]
first = lambda pat: next(((s - t0) / 1e6 for n, s, e in seg if re.search(pat, n)), float("nan"))
fwd_end, replay = first(r"k_time_chunk"), first(r"FBnBwdApply")
print(f"step wall {(t1 - t0) / 1e6:.2f} ms   forward end {fwd_end:.2f} ms   replay start {replay:.2f} ms   replay length {(t1 - t0) / 1e6 - replay:.2f} ms")
fam = {"tile 16x16x128, 8 waves": r"k_conv_hx.*(Li16ELi16ELi128ELi4ELi2E|16, 16, 128, 4, 2,)", "tile 16x16x128, co-resident": r"k_conv_hx.*(Li16ELi16ELi128ELi4ELi1E|16, 16, 128, 4, 1,)",
       "k_wgrad_hx": r"k_wgrad_hx"}
for k, pat in fam.items():
    d = [(e - s) for n, s, e in seg if re.search(pat, n)]
    print(f"{k:30s} {len(d):5d} launches {sum(d) / 1e6:8.2f} ms")

#!/usr/bin/env python3
"""Start / end of every kernel of three consecutive steady-state steps of bench.py, grouped by queue, from a
rocprofv3 --kernel-trace csv directory:

    python tools/step_timeline.py TRACE_DIR OUT.json

A step is taken from the start of one k_msk launch to the start of the next.  Times are microseconds from the start of
the first of the three recoveries.  "summary" says, per step, where the bit tail (if the run has one) lies relative to
the next recovery and the next k_fs_est, and how much of the step neither k_msk nor the kernels of the sample-pass queue
(the one k_agcw / the correlator run on) cover."""
import csv
import glob
import json
import sys


def short(name):
    return name.replace("void ", "").split("(")[0]


def union_len(iv):
    tot, end = 0, None
    for a, b in sorted(iv):
        if end is None or a > end:
            tot += b - a
            end = b
        elif b > end:
            tot += b - end
            end = b
    return tot


def clip(iv, lo, hi):
    return [(max(a, lo), min(b, hi)) for a, b in iv if min(b, hi) > max(a, lo)]


def main():
    rows = []
    for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            q = "queue %s" % r.get("Queue_Id", "?")
            if r.get("Stream_Id") not in (None, ""):
                q += " / stream %s" % r["Stream_Id"]
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), q))
    rows.sort()
    msk = [r for r in rows if r[2].startswith("k_msk<")]
    i0 = len(msk) - 12  # well behind the warm-up, a few steps before the end
    t0 = msk[i0][0]
    t3 = msk[i0 + 3][0]
    lead = 400000  # (ns) what precedes the first recovery: that step's sample passes
    sel = [r for r in rows if r[1] > t0 - lead and r[0] < t3 + lead and not r[2].startswith("at::") and not r[2].startswith("__amd")]
    us = lambda t: round((t - t0) / 1e3, 1)
    queues = {}
    for a, b, n, q in sel:
        queues.setdefault(q, []).append({"kernel": n, "start_us": us(a), "end_us": us(b)})
    main_q = next((q for a, b, n, q in sel if n.startswith("k_agcw") or n.startswith("k_corr4")), None)
    summary = []
    for k in range(3):
        lo, hi = msk[i0 + k][0], msk[i0 + k + 1][0]
        m_iv = clip([(a, b) for a, b, n, q in rows if n.startswith("k_msk<")], lo, hi)
        s_iv = clip([(a, b) for a, b, n, q in rows if q == main_q], lo, hi)
        e = {"step_us": round((hi - lo) / 1e3, 1), "k_msk_us": round(union_len(m_iv) / 1e3, 1),
             "sample_pass_queue_us": round(union_len(s_iv) / 1e3, 1),
             "covered_by_neither_us": round(((hi - lo) - union_len(m_iv + s_iv)) / 1e3, 1)}
        bt = [r for r in rows if r[2] == "k_bittail" and lo <= r[0] < hi + lead]
        # the bit tail of the recovery that ENDS in this step (launched behind it)
        mend = msk[i0 + k][1]
        bt = [r for r in bt if r[0] >= mend]
        if bt:
            a, b = bt[0][0], bt[0][1]
            est = [r for r in rows if r[2] == "k_fs_est" and r[1] > a - lead]
            e["k_bittail"] = {"start_after_k_msk_end_us": round((a - mend) / 1e3, 1), "duration_us": round((b - a) / 1e3, 1),
                              "start_minus_next_k_msk_start_us": round((a - hi) / 1e3, 1),
                              "end_minus_next_k_msk_start_us": round((b - hi) / 1e3, 1)}
            if est:
                e["k_bittail"]["start_minus_nearest_k_fs_est_start_us"] = round((a - min(est, key=lambda r: abs(r[0] - a))[0]) / 1e3, 1)
        else:
            e["k_bittail"] = None
        e["k_msk_end_to_next_k_msk_start_us"] = round((hi - mend) / 1e3, 1)
        summary.append(e)
    json.dump({"source": "rocprofv3 --kernel-trace, bench.py --gpus 1 --steps 50 --warmup 5; three consecutive steps, us from the "
                         "start of the first of their recoveries", "sample_pass_queue": main_q, "summary": summary, "queues": queues},
              open(sys.argv[2], "w"), indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()

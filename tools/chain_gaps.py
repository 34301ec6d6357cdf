"""The C3 chain in a rocprofv3 kernel trace (us): the spans of the world update, the FeAR launch
(fear_v2, or fear_delta_kernel when the obs writer rides in it) and obs_delta_kernel, the two gaps
of the chain per steady step, step_v2(t) end -> FeAR(t) start and FeAR(t) end -> step_v2(t+1)
start, the part of each gap in which no kernel of the process ran at all (idle), and the period.
    python tools/chain_gaps.py run_kernel_trace.csv [last_n_steps]"""
import csv
import statistics as S
import sys


def q(v):
    if not v:
        return "none"
    v = sorted(v)
    return (f"n {len(v):4d}  p10 {v[len(v) // 10]:6.2f}  p50 {S.median(v):6.2f}  "
            f"p90 {v[9 * len(v) // 10]:6.2f}  mean {S.mean(v):6.2f}")


def main(path, n=40):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    every = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows]

    def ks(*subs):
        return [(a, b) for a, b, name in every if any(s in name for s in subs)]

    step, fear, obs = ks("step_v2")[-n:], ks("fear_v2", "fear_delta_kernel")[-n:], ks("obs_delta_kernel")[-n:]

    def idle(a, b):  # the part of [a, b] that no kernel covers
        cover, at = 0, a
        for s, e, _ in every:
            if e <= at or s >= b:
                continue
            s = max(s, at)
            if e > s:
                cover += min(e, b) - s
                at = min(e, b)
        return max(0, b - a - cover)

    print("step_v2 span            ", q([(b - a) / 1e3 for a, b in step]))
    print("FeAR launch span        ", q([(b - a) / 1e3 for a, b in fear]))
    print("obs_delta_kernel span   ", q([(b - a) / 1e3 for a, b in obs]))
    if len(step) == len(fear) and step and step[0][0] < fear[0][0]:
        print("step(t)->fear(t) gap    ", q([(f[0] - s[1]) / 1e3 for s, f in zip(step, fear)]))
        print("   of it idle           ", q([idle(s[1], f[0]) / 1e3 for s, f in zip(step, fear)]))
        print("fear(t)->step(t+1) gap  ", q([(s[0] - f[1]) / 1e3 for f, s in zip(fear, step[1:])]))
        print("   of it idle           ", q([idle(f[1], s[0]) / 1e3 for f, s in zip(fear, step[1:])]))
        print(f"period {(step[-1][0] - step[0][0]) / 1e3 / (len(step) - 1):.2f} us/step over {len(step) - 1} steps")


if __name__ == "__main__":
    main(sys.argv[1], *map(int, sys.argv[2:3]))

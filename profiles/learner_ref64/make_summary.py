"""Writes the tables of profiles/learner_ref64/SUMMARY.md from a run of the sweep:

    python -m pytest tests/test_gpu_learner_shapes.py -m gpu -s --durations=3 > run.log
    python profiles/learner_ref64/make_summary.py run.log > tables.md

The tests print one ``REF64`` JSON line per dense case and one ``REF64D`` line per descriptor update.
Write to a scratch file first: redirecting straight onto SUMMARY.md empties it if this script fails.
The sections after the tables (wall time, negative controls, unmeasured) are written by hand."""
import json
import sys


def read(log):
    rows, drows = [], []
    for line in open(log):
        for tag, dst in (("REF64 ", rows), ("REF64D ", drows)):
            i = line.find(tag)
            if i >= 0 and line[i + len(tag):].startswith("{"):
                dst.append(json.loads(line[i + len(tag):].strip()))
    return rows, drows


def worst_grad(errors):
    """(name, error) of the worst gradient tensor (losses apart)."""
    return max(((n, e) for n, e in errors.items() if not n.endswith(".loss")), key=lambda x: x[1])


def worst_block(r):
    return max(r["blocks"].items(), key=lambda x: x[1]["ratio"])


def table(out, header, lines):
    out.append("| " + " | ".join(header) + " |")
    out.append("|" + "---|" * len(header))
    out.extend("| " + " | ".join(line) + " |" for line in lines)


def main(log):
    rows, drows = read(log)
    if not rows or not drows:
        sys.exit(f"{log}: no REF64 / REF64D lines (run the tests with -s)")
    out = ["# Learner kernels against the float64 reference", "",
           "One run of `tests/test_gpu_learner_shapes.py` on an MI355X (gfx950).  The reference is",
           "`tests/_maddpg_ref64.py` (float64, CPU); `fused` is the kernel under test, `f32 autograd` the torch",
           "composition of the same update (`fused = False`).  Gradient errors are relative L2 per agent, the worst",
           "agent's; a critic loss is relative to its own value per agent, an actor loss to the agent's mean |Q|.",
           "Block errors are `||got - ref|| / (rms(ref[k]) sqrt(block elements))`; the bound of a block check is",
           "4 x the f32 autograd composition's largest block error (floor 1e-6); `ratio` is",
           "fused / max(autograd, 2.5e-7), so a ratio below 4 passes.", "",
           "## Dense fused update (`gw_maddpg_critic_grads` / `gw_maddpg_actor_grads`)", ""]
    lines = []
    for r in rows:
        B = int(r["case"].split("_b")[1])
        fg, ag, wb = worst_grad(r["fused"]), worst_grad(r["autograd"]), worst_block(r)
        lines.append([r["case"], f"{r['masked']} ({B // 8})", f"{fg[1]:.1e} ({fg[0]})", f"{ag[1]:.1e} ({ag[0]})",
                      f"{r['fused']['critic.loss']:.1e} / {r['fused']['actor.loss']:.1e}",
                      f"{r['autograd']['critic.loss']:.1e} / {r['autograd']['actor.loss']:.1e}",
                      f"{r['a_next']:.1e} / {r['probs']:.1e}", f"{wb[1]['ratio']:.2f} ({wb[0]})"])
    table(out, ["case", "masked rows (cap B/8)", "worst gradient: fused", "worst gradient: f32 autograd",
                "critic / actor loss: fused", "critic / actor loss: f32 autograd", "a_next / probs abs (bound 2e-6)",
                "worst block ratio"], lines)
    names = list(rows[0]["fused"])
    out += ["", "Per tensor (`fused` then `f32 autograd`):", ""]
    table(out, ["case"] + names,
          [[r["case"]] + [f"{r['fused'][n]:.1e} {r['autograd'][n]:.1e}" for n in names] for r in rows])
    bn = list(rows[0]["blocks"])
    out += ["", "Largest block error per block check (`fused` / `f32 autograd` / ratio):", ""]
    table(out, ["case"] + bn,
          [[r["case"]] + [f"{r['blocks'][n]['fused']:.1e} / {r['blocks'][n]['autograd']:.1e} / "
                          f"{r['blocks'][n]['ratio']:.2f}" for n in bn] for r in rows])
    out += ["", "## Descriptor learner (`gw_maddpg_desc_update`; two updates per case, an env step between them)", "",
            "`edge rows`: rows with a ReLU input within 1e-5 of zero in float64; their float64 contribution is",
            "subtracted from the gradients of all sides (cap B/8).  Coverage, all three asserted by the test: sampled",
            "rows with `done` set (the next state is the terminal obs, descriptor words 8-11), sampled states that",
            "are reset obs, and the largest number of patched cells of one sampled obs, counted on the dense obs",
            "against the map (N + 1 = 9 on the 6 x 6 map: every patch slot full).", ""]
    lines = []
    for r in drows:
        fg, ag, wb = worst_grad(r["fused"]), worst_grad(r["autograd"]), worst_block(r)
        lines.append([r["case"], str(r["B"]), str(r["update"]), f"{r['edge']} ({r['B'] // 8})", str(r["done"]),
                      str(r["reset"]), str(r["patches"]), f"{fg[1]:.1e} ({fg[0]})", f"{ag[1]:.1e} ({ag[0]})",
                      f"{r['fused']['critic.loss']:.1e} / {r['fused']['actor.loss']:.1e}", f"{r['a_next']:.1e}",
                      f"{wb[1]['ratio']:.2f} ({wb[0]})"])
    table(out, ["case", "B", "update", "edge rows (cap)", "done rows", "reset obs", "max patches",
                "worst gradient: fused", "worst gradient: f32 autograd", "critic / actor loss: fused", "a_next abs",
                "worst block ratio"], lines)
    names = [n for n in drows[0]["fused"] if not n.endswith(".loss")]
    out += ["", "Per tensor, descriptor learner (`fused` then `f32 autograd`):", ""]
    table(out, ["case / update"] + names,
          [[f"{r['case']} / {r['update']}"] + [f"{r['fused'][n]:.1e} {r['autograd'][n]:.1e}" for n in names]
           for r in drows])
    print("\n".join(out))


if __name__ == "__main__":
    main(sys.argv[1])

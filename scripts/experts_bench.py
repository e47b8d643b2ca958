"""Timing of the routed forward of an expert set against its alternatives (profiles/NOTES.md, "game-phase experts").

RISEv2-19, float16x3, batch 256, three differently seeded experts.  Every figure is the host time of descriptor-fed calls that end in
mi_net_wait (submit_boards_gathered: planes built on the GPU, forward, gathered priors written to pinned memory), per call, in ms:

  A          one plain net, 256 boards                          (what a single net costs; the plain path is untouched by expert sets)
  B 86/85/85 the expert set, 256 boards of three phases         (three partial forwards side by side)
  B 200/40/16
  C ...      the same three groups submitted to three plain nets, all three in flight, then three waits -- the only way to route per
             board without an expert set; `C serial` waits for each group before it submits the next

The legs are interleaved round by round; the table gives the median over the rounds and the lowest / highest round.

    python scripts/experts_bench.py [--rounds 12] [--calls 200] [--out experts_bench.txt]
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import experts_cases as ec
    from crazyara_amd import _capi
    from crazyara_amd.neuralnetapi import HipAPI, HipExperts

    lib = _capi.load()
    if lib.mi_device_count() < 1:
        raise SystemExit("no GPU: nothing is measured")
    B = 256
    tmp = tempfile.mkdtemp(prefix="cra_experts_")
    root, dirs = ec.export_experts(tmp, case="risev2-19")
    experts = HipExperts(0, B, root, "float16x3", ec.LICHESS)
    plain = [HipAPI(0, B, d, "float16x3") for d in dirs]
    npol = experts.get_nb_policy_values()
    pools = ec.positions_by_phase((256, 256, 256))

    def loaded(positions):
        buf = ec.CallBuffers(B, npol)
        buf.load(positions)
        return buf, len(positions)

    def submit(net, buf, n):
        if lib.mi_net_submit_boards_gathered(net._h, buf.p_desc, n, 0, buf.p_idx, buf.p_cnt, buf.stride, buf.p_value, buf.p_gath, None):
            raise RuntimeError(_capi.last_error())

    def wait(net):
        if lib.mi_net_wait(net._h):
            raise RuntimeError(_capi.last_error())

    legs = {}
    whole = loaded(ec.make_batch(pools, (86, 85, 85), seed=1))
    legs["A plain net, 256 boards"] = lambda: (submit(plain[0], *whole), wait(plain[0]))
    for counts in ((86, 85, 85), (200, 40, 16)):
        name = "/".join(str(c) for c in counts)
        positions = ec.make_batch(pools, counts, seed=1)
        routed = loaded(positions)
        phases = [p.game_phase(3, ec.LICHESS) for p in positions]
        groups = [loaded([p for p, ph in zip(positions, phases) if ph == e]) for e in range(3)]

        def b(routed=routed):
            submit(experts, *routed)
            wait(experts)

        def c(groups=groups):
            for e in range(3):
                submit(plain[e], *groups[e])
            for e in range(3):
                wait(plain[e])

        def c_serial(groups=groups):
            for e in range(3):
                submit(plain[e], *groups[e])
                wait(plain[e])
        legs["B routed %s" % name] = b
        legs["C three plain nets %s" % name] = c
        legs["C serial %s" % name] = c_serial

    for fn in legs.values():                       # every shape of the timed window, warmed up
        for _ in range(20):
            fn()
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            ms[k].append((time.perf_counter() - t0) * 1e3 / args.calls)
    lines = ["RISEv2-19 float16x3 batch 256, %d rounds x %d calls per leg, ms per call (median, lowest .. highest round)" % (args.rounds, args.calls)]
    for k, v in ms.items():
        lines.append("%-36s %.4f   (%.4f .. %.4f)" % (k, statistics.median(v), min(v), max(v)))
    a = statistics.median(ms["A plain net, 256 boards"])
    for name in ("86/85/85", "200/40/16"):
        bm, cm = statistics.median(ms["B routed " + name]), statistics.median(ms["C three plain nets " + name])
        lines.append("%s: B / A = %.3f   B / C = %.3f" % (name, bm / a, bm / cm))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    experts.close()
    for n in plain:
        n.close()
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()

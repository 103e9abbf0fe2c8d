"""The critic head at the C2 minibatch (B = 65 536): K16Q (64-row tiles, xpa_head_gemm_s3q_critic_mask) against the
256-row split-GEMM block — the plain K40 GEMM on the same x and planes (the gate: K40H without its epilogue) and K40H
itself (xpa_s3_head_critic_mask under xpa_head_critic_form(1)).  One process; every form is captured as a graph of
`--launches` back-to-back launches and the graphs are replayed alternately, `--rounds` samples each.

    python tools/critic_rows256_ab.py [--launches 50] [--rounds 6] [--out profiles/critic_rows256_ab.json --key gate]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--out", default=None, help="JSON file to merge the result into")
    ap.add_argument("--key", default="kernel_ab", help="key of the result inside --out")
    a = ap.parse_args()
    import torch
    from xuanpolicy_amd import graphs, ops
    L = ops.lib()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    # tools/head_conc.py's arguments
    B, H, K = a.batch, 256, 6
    R = 4 * B
    x = torch.randn(B, H, device=dev, generator=g)
    whc = torch.randn(H, H, device=dev, generator=g) * 0.06
    bhc = torch.randn(H, device=dev, generator=g) * 0.1
    wc, bc = torch.randn(1, H, device=dev, generator=g) * 0.06, torch.zeros(1, device=dev)
    ret = torch.randn(R, device=dev, generator=g)
    idx = torch.randperm(R, device=dev)[:B]
    ws = ops.HeadWorkspace(B, K, dev, paired=True)
    W = ws.loss_partials.shape[1]
    wsc = ops.s3_split(whc.t())
    mask = torch.empty((B, 8), dtype=torch.int32, device=dev)
    dv = torch.empty((B,), device=dev)
    c = torch.empty((B, H), device=dev)
    p = ops._p

    def head(fn):
        def run():
            assert fn(1, B, H, p(x), H, p(wsc), p(bhc), 2 * H, p(wc), p(bc), 0.01, p(idx), R, p(ret), 0.25, None,
                      p(ws.p_dw_critic), p(ws.p_dbh_critic), p(ws.p_dbo_critic), p(ws.loss_partials), W, ops._stream(dev),
                      p(mask), p(dv)) == 0
        return run

    def gemm():
        assert L.xpa_s3_gemm(p(x), H, p(wsc), p(c), H, B, H, H, ops._stream(dev)) == 0

    # name -> (launch, xpa_s3_probe mask while it is recorded: 256 = the ping-pong k loop)
    forms = {"k16q_critic_mask": (head(L.xpa_head_gemm_s3q_critic_mask), 0), "k40_gemm_only": (gemm, 0),
             "k40_gemm_only_pp": (gemm, 256)}
    if hasattr(L, "xpa_s3_head_critic_mask"):
        L.xpa_head_critic_form(1)
        forms["k40h_critic_mask"] = (head(L.xpa_s3_head_critic_mask), 0)
    recorded = {}
    for name, (fn, probe) in forms.items():
        L.xpa_s3_probe(probe)
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        recorded[name], _ = graphs.capture(lambda fn=fn: [fn() for _ in range(a.launches)] and None)
        recorded[name].replay()
        L.xpa_s3_probe(0)
    torch.cuda.synchronize()
    res = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name, gr in recorded.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(round(e0.elapsed_time(e1) * 1000 / a.launches, 2))
    out = {"batch": B, "launches_per_graph": a.launches, "unit": "us per launch", "samples": res,
           "median": {n: sorted(v)[len(v) // 2] for n, v in res.items()}}
    print(json.dumps(out), flush=True)
    if a.out:
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc[a.key] = out
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""tests/golden/step_plan.json from a kernel trace of the train step (tools/step_trace.py under rocprofv3 --kernel-trace,
reduced by tools/trace_launches.py): for every traced step, its launches as [label, grid in workgroups, workgroup
size, kernel instance].  The labels are the step's TGNX_LAUNCH_CHECK names in launch order (tgnx._lib.STEP_LABELS);
the kernel instance numbers are include/tgnx.h's TGNX_TGN_AGG_* / _PRED_* / _ATTB_* / _FIXUP_*.  Steps with the same
launches share one entry of `launch_lists`; a case names its config, mode and launch list by index.  The trace's
LDS column is left out: it is the kernel's static segment rounded to 512 bytes, not the dynamic bytes of a launch.  tgn_adam at the head of a step (tgnx_tgn_train_fwd_bwd_pp
with apply_prev) is not one of the step's launches and is dropped.

    python tools/step_plan_golden.py <cases.json> <launches.txt> tests/golden/step_plan.json"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tgb-tgn-dgl_amd"))
LINE = re.compile(r"grid\s+(\d+)x1x1 wg\s+(\d+)x1x1 lds\s+(\d+)\s+(.*)")
ATTB = {("10", "4"): 0, ("16", "4"): 1, ("10", "1"): 2, ("16", "1"): 3}


def classify(name, seen, two):
    """(label, kernel instance) of a traced kernel, given the labels already seen in its step"""
    def has(*ws):
        return all(w in name for w in ws)
    if has("tgn_mark<true>"):
        return "tgn_mark", 0
    if has("tgn_scan<true>"):
        return ("tgn_scan_next" if "tgn_fixup_update" in seen else "tgn_scan_early" if "tgn_wgrad3" in seen
                else "tgn_scan"), 0
    if has("tgn_gather("):
        return "tgn_gather", 0
    if has("tgn_enc_fill"):
        return "tgn_agg_emit", 0
    m = re.search(r"tgn_agg_emit<(-?\d+), (true|false)>", name)
    if m:
        if m.group(2) == "true":
            return "tgn_emb_update", 0
        return "tgn_agg_emit", {"0": 1, "1": 2, "-1": 3}[m.group(1)]
    if has("RingMergeJob"):
        return "tgn_gru_edge", 0 if "gemmN_kernel_w<" in name else 1
    if has("gemmN_kernel<", "LoadZ,", "EpiProj") and not has("LoadProjWT"):
        return "tgn_proj", 0
    if has("tgn_attn_fwd<true>"):
        return ("tgn_attn_fwd2" if "tgn_attn_fwd" in seen else "tgn_attn_fwd"), 0
    if has("gemm_kernel<", "EpiProj"):
        return "tgn_proj2", 0
    m = re.search(r"tgn_pred_train<(true|false), (\d+)>", name)
    if m:
        return "tgn_pred_train", 2 if m.group(1) == "false" else 0 if m.group(2) == "10" else 1
    if has("gemm_kernel<", "LoadGruA"):
        return "tgn_emb_update_gru", 0
    m = re.search(r"tgn_attn_bwd<(\d+), (\d+)>", name)
    if m:
        return ("tgn_attn_bwd2" if two and "tgn_attn_bwd2" not in seen else "tgn_attn_bwd"), ATTB[m.groups()]
    if has("KvReduceJob"):
        return "tgn_kv_reduce2", 0
    if has("StoreJob"):
        return "tgn_wgrad3", 1 if "ScanJob" in name else 0
    if has("gemmN_kernel<", "LoadLpA"):
        return "tgn_wgrad_dz0", 1 if "ScanJob" in name else 0
    if has("gemmN_kernel<", "LoadProjWT", "LoadZ1T"):
        return "tgn_dh1", 0
    if has("gemm_fixup_kernel<"):
        if "TrainTail<true>" in name:
            return "tgn_fixup_update", 1
        return "tgn_fixup_update", 2 if name.count("GemmFix<") == 12 else 0
    raise ValueError("no label for " + name)


def main(cases_path, launches_path, out_path):
    from tgnx._lib import STEP_LABELS
    cases = json.load(open(cases_path))
    rows = [LINE.match(l).groups() for l in open(launches_path).read().splitlines()]
    seps = [i for i, (g, w, _, n) in enumerate(rows) if g == "256" and "ring_reset_kernel" in n]
    assert len(seps) == 2 * len(cases), (len(seps), len(cases))
    out, seen_keys = [], set()
    for n, cs in enumerate(cases):
        key = json.dumps(cs, sort_keys=True)
        launches, seen = [], []
        for g, w, lds, name in rows[seps[2 * n] + 1:seps[2 * n + 1]]:
            if "tgn_adam" in name:
                continue
            label, kern = classify(name, seen, cs["layers"] == 2)
            assert not seen or STEP_LABELS.index(label) > STEP_LABELS.index(seen[-1]), (cs, seen, label)
            assert int(g) % int(w) == 0
            seen.append(label)
            launches.append([STEP_LABELS.index(label), int(g) // int(w), int(w), kern])
        cs = dict(cs)
        cs.pop("step")
        key = json.dumps(cs, sort_keys=True)
        if key in seen_keys:   # (the two steps of a mode that does not prefetch: the same launches twice)
            assert [c for c in out if c["case"] == cs][0]["launches"] == launches, cs
            continue
        seen_keys.add(key)
        out.append({"case": cs, "launches": launches})
    cfg_fields = [k for k in out[0]["case"] if k not in ("mode", "world", "prefetched", "parity")]
    configs, modes, lists = [], [], []
    for c in out:
        cfg = [c["case"][k] for k in cfg_fields]
        for table, x in ((configs, cfg), (modes, [c["case"]["mode"], c["case"]["world"]]), (lists, c["launches"])):
            if x not in table:
                table.append(x)
    rows = [[configs.index([c["case"][k] for k in cfg_fields]), modes.index([c["case"]["mode"], c["case"]["world"]]),
             c["case"]["prefetched"], c["case"]["parity"], lists.index(c["launches"])] for c in out]
    dump = lambda x: json.dumps(x, separators=(",", ":"))

    def wrap(items, width=150):   # a JSON list's items, several to a line
        lines, cur = [], ""
        for it in map(dump, items):
            if cur and len(cur) + len(it) + 1 > width:
                lines.append(cur)
                cur = ""
            cur += ("," if cur else "") + it
        return ",\n".join(lines + [cur])
    with open(out_path, "w") as f:
        f.write('{"labels":%s,\n "record":["label","grid","block","kernel"],\n "launch_lists":[\n%s],\n'
                % (dump(list(STEP_LABELS)), wrap(lists)))
        f.write(' "config_fields":%s,\n "configs":[\n%s],\n "modes":%s,\n' % (dump(cfg_fields), wrap(configs), dump(modes)))
        f.write(' "case_fields":["config","mode","prefetched","parity","launch_list"],\n "cases":[\n%s]}\n' % wrap(rows))
    print(len(cases), "traced steps ->", len(out), "distinct cases")


if __name__ == "__main__":
    main(*sys.argv[1:4])

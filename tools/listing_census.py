"""Static census of one solve kernel's gfx950 listing by source function.

Compile the device code to assembly with line tables (the product's flags plus
`-S --cuda-device-only -gline-tables-only`), then
    python tools/listing_census.py LISTING.s [kernel-substring [csrc-dir]]
(defaults: solve_group_kernelILi128ELi96E, this tree's csrc; give the csrc directory the listing was
compiled from when it is another commit's).
Every instruction is attributed to the innermost frame of its `.loc` inline chain that lies in one
of the functions of FUNCS (so a helper inlined into ldl_apply counts for ldl_apply, and ldl_apply
inlined into admm_iteration for ldl_apply alone), and counted by class.  The counts are static:
they say what the compiler emitted, not how often it runs."""
import re
import sys
from collections import Counter, defaultdict
from pathlib import Path

CSRC = Path(__file__).resolve().parents[1] / "convex-mpc-unitree-go2_amd" / "csrc"
# function -> (file, group it is reported under)
FUNCS = {
    "ldl_apply": ("cmpc_factor.h", "ldl_apply"),
    "gradient": ("cmpc_gradient.h", "gradient"),
    "gradient_powers": ("cmpc_gradient.h", "gradient"),
    "admm_iteration": ("cmpc_solve.h", "admm_iteration (rest)"),
    "ldl_tiles": ("cmpc_factor.h", "ldl_tiles + sweep"),
    "sweep_publish": ("cmpc_factor.h", "ldl_tiles + sweep"),
    "sweep_operands": ("cmpc_factor.h", "ldl_tiles + sweep"),
    "sweep_mfma": ("cmpc_factor.h", "ldl_tiles + sweep"),
    "sweep_diagfix": ("cmpc_factor.h", "ldl_tiles + sweep"),
    "sweep_block": ("cmpc_factor.h", "ldl_tiles + sweep"),
    "sweep_block_plain": ("cmpc_factor.h", "ldl_tiles + sweep"),
    "pivot_block": ("cmpc_factor.h", "ldl_tiles + sweep"),
    "panel_row": ("cmpc_factor.h", "ldl_tiles + sweep"),
    "scale_tile": ("cmpc_factor.h", "ldl_tiles + sweep"),
    "diag_element": ("cmpc_factor.h", "ldl_tiles + sweep"),
    "condense_tiles_nil": ("cmpc_condense.h", "condense_tiles_nil"),
    "step_sums": ("cmpc_condense.h", "condense_tiles_nil"),
    "mirror_diagonals": ("cmpc_condense.h", "mirror_diagonals"),
    "condense_finish": ("cmpc_condense.h", "condense_finish"),
    "polish_check": ("cmpc_polish.h", "polish_check"),
    "polish_setup": ("cmpc_polish.h", "polish_setup"),
    "stage_instance": ("cmpc_solve.h", "stage_instance"),
    # what an instance runs once, or once per polish session
    "build_admm_basis": ("cmpc_polish.h", "build_admm_basis"),
    "nilpotent_step": ("cmpc_condense.h", "nilpotent_step"),
    "starting_point": ("cmpc_solve.h", "starting_point"),
    "solve_instance": ("cmpc_solve.h", "solve_instance"),
    "drain_bin": ("cmpc_solve.h", "drain_bin"),
    "instance_terrain": ("cmpc_instance.h", "instance_terrain"),
    "force_triple": ("cmpc_solve.h", "output writers"),
    "write_w": ("cmpc_solve.h", "output writers"),
    "write_y": ("cmpc_solve.h", "output writers"),
    "write_lam": ("cmpc_solve.h", "output writers"),
}


def function_ranges(csrc=CSRC):
    """(file, first line, last line, group) of every function of FUNCS: from its name's line to
    the line before the next function definition of that file."""
    out = []
    for fn in sorted({f for f, _ in FUNCS.values()}):
        lines = (Path(csrc) / fn).read_text().splitlines()
        starts = []
        for i, ln in enumerate(lines, 1):
            m = re.match(r"^(?:__device__|__global__|static|inline|constexpr)[^;]*?\b(\w+)\s*\($", ln) or \
                re.match(r"^(?:__device__|__global__)[^;=]*?\b(\w+)\s*\(", ln)
            if m:
                starts.append((i, m.group(1)))
        for (a, name), nxt in zip(starts, starts[1:] + [(len(lines) + 1, None)]):
            if name in FUNCS and FUNCS[name][0] == fn:
                out.append((fn, a, nxt[0] - 1, FUNCS[name][1]))
    return out


def classify(op):
    if op.startswith("v_mfma"):
        return "MFMA"
    if op in ("s_waitcnt", "s_nop") or op.startswith("s_waitcnt"):
        return "wait/nop"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "scratch_", "flat_")):
        return "VMEM"
    if op.startswith("s_"):
        return "SALU"
    return "other"


def main():
    lst = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "solve_group_kernelILi128ELi96E"
    ranges = function_ranges(sys.argv[3] if len(sys.argv) > 3 else CSRC)
    cls, extra = defaultdict(Counter), defaultdict(Counter)
    inside, group, total = False, "(other)", 0
    frame = re.compile(r"([\w.]+):(\d+):\d+")
    with open(lst, errors="replace") as f:
        for ln in f:
            if not inside:
                if ln.startswith("_Z") and want in ln and ln.rstrip().split(";")[0].rstrip().endswith(":"):
                    inside = True
                continue
            if ln.startswith(".Lfunc_end"):
                break
            s = ln.strip()
            if s.startswith(".loc"):
                group = "(other)"
                for fn, line in frame.findall(s.split(";", 1)[1] if ";" in s else ""):
                    hit = [g for f2, a, b, g in ranges if f2 == fn and a <= int(line) <= b]
                    if hit:
                        group = hit[0]
                        break
                continue
            if not s or s[0] in ".;" or s.endswith(":"):
                continue
            op = s.split()[0]
            if not re.match(r"^[a-z]+_", op):
                continue
            total += 1
            cls[group][classify(op)] += 1
            e = extra[group]
            e["saveexec"] += "saveexec" in op
            e["cond branch"] += op.startswith("s_cbranch")
            e["s_nop"] += op == "s_nop"
            e["v_cndmask"] += op.startswith("v_cndmask")
            e["dpp"] += "dpp" in s.split(";")[0]
            e["v_div_*"] += op.startswith(("v_div_scale", "v_div_fmas", "v_div_fixup"))
            if op.startswith("ds_"):
                e["LDS " + op] += 1
    print(f"kernel *{want}*: {total} instructions")
    order = ["VALU", "MFMA", "SALU", "LDS", "VMEM", "branch", "wait/nop", "other"]
    for g in sorted(cls, key=lambda k: -sum(cls[k].values())):
        c = cls[g]
        print(f"{g}: {sum(c.values())}  " + "  ".join(f"{k} {c[k]}" for k in order if c[k]))
        e = extra[g]
        print("    " + "  ".join(f"{k} {e[k]}" for k in ("saveexec", "cond branch", "s_nop", "v_cndmask",
                                                          "dpp", "v_div_*")))
        lds = {k[4:]: v for k, v in e.items() if k.startswith("LDS ") and v}
        if lds:
            print("    " + "  ".join(f"{k} {v}" for k, v in sorted(lds.items())))


if __name__ == "__main__":
    main()

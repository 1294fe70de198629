"""Static per-wave instruction counts of one kernel in a gfx950 assembly file:
whole-kernel totals of the opcode families DESIGN section 3 tabulates, and the
VALU / MFMA / LDS counts of every segment between two s_barrier instructions,
in program order.

usage: hipcc <product flags> --cuda-device-only -S csrc/ffn.hip -o ffn.s
       python scripts/kernel_valu_counts.py ffn.s conv_chain_kernelILi1E [--segments]"""
import collections
import re
import sys


def kernel_body(text, key):
    """Instruction mnemonics of the first kernel whose mangled name contains `key`."""
    m = re.search(r"^(\S*%s\S*):" % re.escape(key), text, re.M)
    if not m:
        raise SystemExit(f"no kernel matching {key}")
    end = text.index(".end_amdhsa_kernel", m.end()) if ".end_amdhsa_kernel" in text[m.end():] else len(text)
    body = text[m.end():end]
    stop = body.find("s_endpgm")
    # the kernel may hold several s_endpgm (early returns): keep up to the .section / .rodata that follows
    sec = re.search(r"^\s*\.(section|rodata|p2align\s+6)", body, re.M)
    if sec:
        body = body[:sec.start()]
    elif stop >= 0:
        body = body[:stop]
    ops = []
    for line in body.splitlines():
        line = line.split(";")[0].strip()
        if not line or line.startswith(".") or line.endswith(":"):
            continue
        ops.append(line.split()[0])
    return m.group(1), ops


def family(op):
    if "mfma" in op:
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("s_"):
        return "salu"
    return "vmem"


def main():
    text = open(sys.argv[1]).read()
    name, ops = kernel_body(text, sys.argv[2])
    c = collections.Counter(ops)
    fam = collections.Counter(family(o) for o in ops)
    print(f"{name[:80]}: {len(ops)} instructions, VALU {fam['valu']}, MFMA {fam['mfma']}, SALU {fam['salu']}, "
          f"LDS {fam['lds']}")

    def tot(pred):
        return sum(n for o, n in c.items() if pred(o))

    rows = [("v_sqrt_f32", lambda o: o.startswith("v_sqrt_f32")), ("v_rsq_f32", lambda o: o.startswith("v_rsq_f32")),
            ("v_div_scale/fmas/fixup", lambda o: o.startswith("v_div_")), ("v_rcp_f32", lambda o: o.startswith("v_rcp_f32")),
            ("v_exp_f32", lambda o: o.startswith("v_exp_f32")), ("v_mov_b32", lambda o: o.startswith("v_mov_b32")),
            ("v_cndmask", lambda o: o.startswith("v_cndmask")), ("v_add_f32", lambda o: o.startswith("v_add_f32")),
            ("v_sub_f32", lambda o: o.startswith("v_sub")  and "f32" in o), ("v_mul_f32", lambda o: o.startswith("v_mul_f32")),
            ("v_fma/fmac_f32", lambda o: o.startswith(("v_fma_f32", "v_fmac_f32"))),
            ("v_pk_add_f32", lambda o: o.startswith("v_pk_add_f32")), ("v_pk_mul_f32", lambda o: o.startswith("v_pk_mul_f32")),
            ("v_pk_fma_f32", lambda o: o.startswith("v_pk_fma_f32")), ("v_dot2", lambda o: o.startswith("v_dot2")),
            ("ds_bpermute", lambda o: o.startswith("ds_bpermute")), ("ds_read_u16", lambda o: o.startswith("ds_read_u16"))]
    for label, pred in rows:
        print(f"  {label:24s} {tot(pred)}")
    if "--segments" in sys.argv:
        seg = collections.Counter()
        i = 0
        for o in ops:
            if o == "s_barrier":
                print(f"  segment {i:2d}: VALU {seg['valu']:4d} MFMA {seg['mfma']:3d} LDS {seg['lds']:3d} "
                      f"SALU {seg['salu']:4d} VMEM {seg['vmem']:3d}")
                seg = collections.Counter()
                i += 1
            else:
                seg[family(o)] += 1
        print(f"  segment {i:2d}: VALU {seg['valu']:4d} MFMA {seg['mfma']:3d} LDS {seg['lds']:3d} "
              f"SALU {seg['salu']:4d} VMEM {seg['vmem']:3d}")


if __name__ == "__main__":
    main()

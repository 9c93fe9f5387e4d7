"""Instruction counts of the tile loop of k_z_pair_pipe from the device assembly of csrc/fft_native_yz.hip:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I image-preprocessing-pipeline_amd/csrc -S --cuda-device-only \
        image-preprocessing-pipeline_amd/csrc/fft_native_yz.hip -o yz.s
    python profiles/zpass_count.py yz.s [more.s ...]

Per factored instantiation of 256-, 512- and 1024-point lines (and per form, full grid / predicated, where the source has both): the
instructions between the head of the tile loop -- the backward branch with the longest span -- and that branch, how many of them are
VALU (v_*) and packed (v_pk_*), and the kernel's registers, LDS, scratch and occupancy from its descriptor."""
import re
import sys


def kernels(text):
    """mangled name -> lines from the kernel's label to its descriptor's end"""
    parts = re.split(r"^(_ZN2mi[^\s:]*k_z_pair_pipe[^\s:]*):\s*(?:;.*)?$", text, flags=re.M)
    out = {}
    for i in range(1, len(parts) - 1, 2):
        end = parts[i + 1].find(".end_amdhsa_kernel")
        if end >= 0:
            out[parts[i]] = parts[i + 1][:end].splitlines()
    return out


def count(lines):
    label_at, insts = {}, []
    for ln in lines:
        s = ln.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            label_at[m.group(1)] = len(insts)
        elif s and not s.startswith((";", ".")):
            insts.append(s.split(";")[0].strip())
    span, lo, hi = 0, 0, 0
    for i, ins in enumerate(insts):
        m = re.match(r"^s_c?branch\w*\s+(\.LBB\d+_\d+)", ins)
        tgt = label_at.get(m.group(1)) if m else None
        if tgt is not None and tgt <= i and i - tgt > span:
            span, lo, hi = i - tgt, tgt, i
    op = [b.split()[0] for b in insts[lo:hi + 1]]
    n = lambda *pre: sum(o.startswith(pre) for o in op)  # noqa: E731
    return dict(loop=len(op), valu=n("v_"), packed=n("v_pk_"), lds=n("ds_"), salu=n("s_"), vmem=n("global_", "buffer_", "flat_"))


def descriptor(lines):
    t = "\n".join(lines)
    get = lambda k: (re.search(r"\.amdhsa_" + k + r"\s+(\d+)", t) or [None, "?"])[1]  # noqa: E731
    return dict(vgpr=get("next_free_vgpr"), sgpr=get("next_free_sgpr"), lds=get("group_segment_fixed_size"), scratch=get("private_segment_fixed_size"))


def main():
    for path in sys.argv[1:]:
        text = open(path).read()
        print(path)
        for name, lines in sorted(kernels(text).items()):
            # <LZ2, 1, REALG = true, 512, 8, PHL = true, TOPON = true, FACT = true[, FULLZ]>
            m = re.search(r"k_z_pair_pipeILi(\d+)ELi1ELb1ELi512ELi8ELb1ELb1ELb1E(Lb([01])E)?E", name)
            if not m or int(m.group(1)) not in (8, 9, 10):
                continue
            form = {None: "", "1": " full grid", "0": " predicated"}[m.group(3)]
            c, t = count(lines), descriptor(lines)
            o = re.search(r"; Occupancy: (\d+)", text[text.find(name + ":"):])  # (the comment block behind the kernel)
            print(f"  {1 << int(m.group(1)):5d} points{form:11s} loop {c['loop']:5d}  VALU {c['valu']:5d}  packed {c['packed']:5d}  LDS {c['lds']:4d}  SALU {c['salu']:4d}  "
                  f"VMEM {c['vmem']:3d}  VGPRs {t['vgpr']}  SGPRs {t['sgpr']}  static LDS {t['lds']}  scratch {t['scratch']}  occupancy {o.group(1) if o else '?'}")


if __name__ == "__main__":
    main()

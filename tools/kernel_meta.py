"""Per-kernel comparison of two builds of libjr.so (or of two objects of one
source file): the code objects' notes (VGPRs, spills, scratch, LDS) and
their disassembly (MFMA, LDS-DMA, LDS-read, s_barrier and s_waitcnt vmcnt(0)
counts, total instructions).

    python tools/kernel_meta.py <old> <new> [substring of the kernel names, default k_conv]

Conditions a refactor of kernel code must hold, each the old build's own
value; the exit status is 1 when one is broken:
  * the same kernel symbols;
  * no more VGPR spills or scratch than before, so 0 wherever the old build
    has 0.  (Stated for the conv refactor as "0 in both builds"; that cannot
    be met as written: the old build itself spills in 29 k_conv_bf16 kernels,
    mostly stream-K 256x256 tiles, and those are listed on every run.)
  * equal LDS bytes;
  * no kernel crosses a waves-per-SIMD step -- a register budget that crosses
    one (256 -> 257 VGPRs: 2 -> 1 waves per SIMD) is what made the first
    counting stream-K hand-off 8 % slower;
  * equal MFMA, LDS-DMA, LDS-read and s_barrier counts per kernel;
  * no more s_waitcnt vmcnt(0) than before (csrc/jr_conv_impl.h dma16_ring:
    a drain in the steady K loop empties the DMA ring every K-tile).
Reported without a bound: the per-kernel VGPR and instruction-count deltas.
"""
import collections
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"
COUNTS = {"mfma": r"\bv_mfma_", "lds_dma": r"\b(global|buffer)_load_lds_|\bbuffer_load_\w+.* lds\b",
          "lds_read": r"\bds_(read|load)", "barrier": r"\bs_barrier\b", "vmcnt0": r"\bs_waitcnt\b.*vmcnt\(0\)"}


def waves_per_simd(vgprs):
    """gfx950: 512 unified VGPRs per SIMD lane, allocated in blocks of 8, at most 8 waves."""
    return min(8, 512 // max(8, -(-vgprs // 8) * 8))


def code_objects(path, tmp):
    """The gfx950 code objects bundled into a .so / .o, unbundled into tmp."""
    fat = os.path.join(tmp, "fat.bin")
    subprocess.run([LLVM + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, path, "/dev/null"], check=True)
    data = open(fat, "rb").read()
    idx = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), data)]
    for k, i in enumerate(idx):
        j = idx[k + 1] if k + 1 < len(idx) else len(data)
        bundle, co = f"{tmp}/b{k}.bin", f"{tmp}/c{k}.co"
        open(bundle, "wb").write(data[i:j])
        r = subprocess.run([LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + bundle,
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], capture_output=True)
        if r.returncode == 0:
            yield co


def meta(path):
    """{kernel symbol: {vgpr, spill, scratch, lds, instr, mfma, ...}}"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(path, tmp):
            notes = subprocess.run([LLVM + "llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            for blk in notes.split("  - .agpr_count")[1:]:
                f = {k: re.search(r"\.%s:\s+(\S+)" % k, blk) for k in
                     ("name", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
                if not (f["name"] and f["vgpr_count"]):
                    continue
                num = lambda k: int(f[k].group(1)) if f[k] else 0  # noqa: E731
                out[f["name"].group(1)] = {"vgpr": num("vgpr_count"), "lds": num("group_segment_fixed_size"),
                                           "spill": num("vgpr_spill_count"),
                                           "scratch": num("private_segment_fixed_size"),
                                           **{k: 0 for k in COUNTS}, "instr": 0, "sha": hashlib.sha256()}
            asm = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True,
                                 text=True).stdout
            cur = None
            for line in asm.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    cur = out.get(m.group(1))
                elif cur is not None and line.startswith("\t"):
                    text = line.split("//")[0].strip()
                    cur["instr"] += 1
                    cur["sha"].update(text.encode())
                    for k, rx in COUNTS.items():
                        cur[k] += bool(re.search(rx, text))
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, r))


def main(old, new, pat="k_conv"):
    a = {n: v for n, v in meta(old).items() if pat in n}
    b = {n: v for n, v in meta(new).items() if pat in n}
    both = sorted(set(a) & set(b))
    short = demangle(both)
    broken = [f"kernel only in {w}: {n}" for w, s in (("old", set(a) - set(b)), ("new", set(b) - set(a))) for n in s]
    for n in both:
        x, y = a[n], b[n]
        why = [f"{k} {x[k]} -> {y[k]}" for k in ("lds", "mfma", "lds_dma", "lds_read", "barrier") if x[k] != y[k]]
        why += [f"{k} {x[k]} -> {y[k]}" for k in ("spill", "scratch") if y[k] > x[k]]
        if y["vmcnt0"] > x["vmcnt0"]:
            why.append(f"vmcnt0 {x['vmcnt0']} -> {y['vmcnt0']}")
        if waves_per_simd(x["vgpr"]) != waves_per_simd(y["vgpr"]):
            why.append(f"waves/SIMD {waves_per_simd(x['vgpr'])} -> {waves_per_simd(y['vgpr'])} "
                       f"(vgpr {x['vgpr']} -> {y['vgpr']})")
        broken += [f"{short[n][:110]}: {w}" for w in why]
    same = sum(a[n]["sha"].digest() == b[n]["sha"].digest() for n in both)
    print(f"{len(both)} kernels in both builds, {same} with identical instruction text; "
          f"{len(broken)} broken conditions")
    for line in broken:
        print("  BROKEN", line)
    for n in both:
        if a[n]["spill"] or a[n]["scratch"]:
            print(f"  (old build: spill {a[n]['spill']} scratch {a[n]['scratch']}; new: {b[n]['spill']} "
                  f"{b[n]['scratch']})  {short[n][:110]}")
    for key in ("vgpr", "instr", "vmcnt0"):
        d = collections.Counter(b[n][key] - a[n][key] for n in both)
        print(f"{key} delta (new - old): count per delta", dict(sorted(d.items())))
        for n in sorted(both, key=lambda n: -abs(b[n][key] - a[n][key]))[:4]:
            if b[n][key] != a[n][key]:
                print(f"  {a[n][key]} -> {b[n][key]}  {short[n][:110]}")
    print("instructions, total:", sum(a[n]["instr"] for n in both), "->", sum(b[n]["instr"] for n in both))
    return 1 if broken else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:4]))

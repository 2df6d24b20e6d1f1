#!/bin/bash
# Registers / scratch / LDS / kernarg size of every kernel in the product .so, from the metadata
# of EVERY gfx950 code object in it (one per .hip translation unit; the bundler tool unbundles
# only the first, so the AMDGPU ELF images are cut out of the file by their headers).  Runs
# without a GPU.
#   kernel_resources.sh [lib.so]            one line per kernel, sorted by demangled name
#   kernel_resources.sh [lib.so] PATTERN    + opcode counts of interest of the kernels whose
#                                           mangled name contains PATTERN
#   kernel_resources.sh --digest [lib.so]   one line per kernel: resources, instruction count and
#                                           a digest of the disassembled instruction stream
#                                           (no addresses, no encodings, no trailing comments).
#                                           Sorted by name, so the outputs of two builds `diff`:
#                                           an equal line = the same machine code
# The summary on stderr counts kernels and code objects and names every kernel that more than
# one code object defines (the tables are keyed by name and show one copy of it).
digest=0
if [ "$1" = "--digest" ]; then digest=1; shift; fi
exec python3 - "${1:-blueberry_amd/libblueberry_hip.so}" "$digest" "${2:-}" <<'PY'
import collections, hashlib, os, re, struct, subprocess, sys, tempfile
so, digest, pat = sys.argv[1], sys.argv[2] == "1", sys.argv[3]
B = "/opt/rocm/lib/llvm/bin/"
run = lambda *a: subprocess.run(a, text=True, capture_output=True, check=True).stdout
blob = open(so, "rb").read()
meta, code = {}, {}          # mangled name -> resources / instruction lines
seen = collections.Counter() # mangled name -> code objects that define it
with tempfile.TemporaryDirectory() as tmp:
    pos = images = 0
    while True:
        pos = blob.find(b"\x7fELF", pos)
        if pos < 0:
            break
        hdr = blob[pos:pos + 64]
        pos += 4
        if len(hdr) < 64 or hdr[4] != 2 or struct.unpack_from("<H", hdr, 18)[0] != 224:
            continue                                   # not a 64-bit EM_AMDGPU image
        shoff, = struct.unpack_from("<Q", hdr, 40)
        shentsize, shnum = struct.unpack_from("<HH", hdr, 58)
        co = os.path.join(tmp, "k%d.co" % images)
        with open(co, "wb") as fh:
            fh.write(blob[pos - 4:pos - 4 + shoff + shentsize * shnum])
        images += 1
        # a kernel's entry runs from its "- .agpr_count:" to the next one (keys are sorted)
        for blk in re.split(r"^\s*- \.agpr_count:", run(B + "llvm-readelf", "--notes", co), flags=re.M)[1:]:
            g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
            name = re.search(r"\.symbol:\s+(\S+)\.kd", blk).group(1)
            seen[name] += 1
            meta[name] = (g("vgpr_count"), g("sgpr_count"), g("private_segment_fixed_size"),
                          g("group_segment_fixed_size"), g("kernarg_segment_size"))
        if digest or pat:
            asm = run(B + "llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co)
            for m in re.finditer(r"^[0-9a-f]* ?<(\S+)>:\n(.*?)(?=^[0-9a-f]* ?<\S+>:\n|\Z)", asm, re.S | re.M):
                lines = [re.sub(r"\s*//.*", "", l).strip() for l in m.group(2).splitlines()]
                # ("...": the zero padding behind a code object's last kernel, not an instruction)
                code[m.group(1)] = [l for l in lines if l and l != "..."]
names = sorted(meta)
try:                         # sorted by demangled name where c++filt is there, else by mangled
    demangled = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), text=True,
                                               capture_output=True, check=True).stdout.splitlines()))
except (OSError, subprocess.CalledProcessError):
    demangled = {k: k for k in names}
for k in sorted(names, key=lambda k: (demangled[k], k)):
    res = "vgpr %-3d sgpr %-3d scratch %-4d lds %-5d kernarg %-4d" % meta[k]
    if digest:
        ins = code.get(k, [])
        res += " insts %-5d %s" % (len(ins), hashlib.sha256("\n".join(ins).encode()).hexdigest()[:16])
    print(res, demangled[k])
for k in sorted(names):
    if pat and pat in k:
        c = collections.Counter(l.split()[0] for l in code.get(k, []))
        keys = ['v_pk_add_f32', 'v_pk_mul_f32', 'v_pk_fma_f32', 'v_rsq_f32', 'v_rsq_f64', 'v_fma_f64',
                'v_mul_f64', 'v_add_f64', 'v_add_f32_dpp', 'v_mov_b32_dpp', 'global_load_dwordx4',
                'buffer_store_dword', 'ds_write_b32', 's_waitcnt', 'scratch_load_dword',
                'scratch_store_dword', 's_load_dwordx8', 'v_readlane_b32', 's_nop']
        print(k[:100], 'total', sum(c.values()), {q: c[q] for q in keys if c[q]})
print("# %d kernels in %d code objects" % (len(names), images), file=sys.stderr)
# the tables above are keyed by name: a kernel compiled into two code objects would show once
twice = sorted(k for k in names if seen[k] > 1)
if twice:
    print("# NOTE: %d kernels are defined in more than one code object (the line above shows one "
          "copy of each):" % len(twice), file=sys.stderr)
    for k in twice:
        print("#   x%d %s" % (seen[k], demangled[k][:120]), file=sys.stderr)
PY

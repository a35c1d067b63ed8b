"""Which kernel a shape gets, pinned on the CPU.

The four shipped GEMM kernels are bit-identical by design, and so are the attention forms of one precision: a routing
mistake passes every numeric test and shows only as lost speed.  This test compiles gemm.hip and attention.hip as they are
into a launch recorder (tests/launch_routes_rec.hip: a host-only build in which a kernel launch prints the kernel
instantiation, its grid, block and dynamic LDS, and the device reports a CU count given on the command line), runs the
shapes of the checkpoint geometries and the labelled rows of the GPU tests through it on 256, 64 and 4 CUs, and compares
with tests/golden/launch_routes.txt.

The golden holds one line per launch for the rows a reader wants to see (the labelled rows, every full-layer GEMM of the
five geometries in fp16, the attention launches of their token counts) and, because one line per launch of every case would
be several MB, one digest line per group of cases for the whole sweep: the cases, launches and refusals of the group, its
launches per kernel family, and a hash of the full records.  A changed route changes a family count, and the failing
assertion names the file the full records of the run were written to.

Regenerate (after a deliberate routing change): MCM_WRITE_LAUNCH_ROUTES=1 python -m pytest tests/test_launch_routes_cpu.py
"""
import ast
import hashlib
import os
import re
import shutil
import subprocess
from collections import Counter

import pytest

from mcm_amd.config import CHECKPOINTS, WIDE_HEAD_CHECKPOINTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_routes.txt")
BF16, F32, F16 = 0, 1, 2
PREC = {"bf16": BF16, "fp32": F32, "fp16": F16}
STORE, GELU, RESID, PATCH, STORE_X2, GELU_X2, GELU_ERF, GELU_ERF_X2 = range(8)
CUS = (256, 64, 4)   # a whole MI355X; a partitioned lease; grid 0 (everything goes to the tile kernels)
BATCHES = (1, 32, 37, 64, 72, 128, 256, 512)
GEOMETRIES = {n: g for n, g in {**CHECKPOINTS, **WIDE_HEAD_CHECKPOINTS}.items()
              if n in ("ViT-B/32", "ViT-B/16", "ViT-L/14", "ViT-L/14@336px", "ViT-H/14-laion2b")}
# (id, precision, split weights, split activations in and out): the operand forms of a tower
FORMS = [("bf16", BF16, 0, 0), ("fp16", F16, 0, 0), ("fp32", F32, 0, 0), ("bf16-W", BF16, 1, 0), ("fp16-W", F16, 1, 0),
         ("fp16-X", F16, 0, 1)]
FAMILY = {"gemm_tile_kernel": "tile128", "gemm_tile64_kernel": "tile64", "gemm_pp_kernel": "pingpong"}


def _gemm(prec, epi, M, N, K, ksplit=0, xsplit=0, px=0, ldx=None, ldo=None):
    """The G line of a logical [M, K] x [N, K] problem (row strides ldx, ldo: dense when not given), with the columns of a
    split weight, a split X and a split output doubled as mcm_api.hip's gemm() and mcm_op_linear_ex double them."""
    x2 = int(epi in (STORE_X2, GELU_X2, GELU_ERF_X2))
    return f"G {prec} {epi} {M} {N} {K << ksplit} {(ldx or K) << xsplit} {(ldo or N) << x2} {ksplit} {xsplit} {px} 0"


def _pad256(M):
    return (M + 255) // 256 * 256


def _tower_gemms(prec, ks, xs, nseq, L, D, ff, erf, cls):
    """The GEMMs of run_layers (mcm_api.hip): a whole-batch layer and, with `cls`, the CLS-only last layer.  A dense problem
    that starts at row 0 of its buffer runs on M padded to whole 256-row tiles (mcm_api.hip gemm()): raw and padded here."""
    store = STORE_X2 if xs else STORE
    act = (GELU_ERF_X2 if xs else GELU_ERF) if erf else (GELU_X2 if xs else GELU)
    M = nseq * L
    for m in sorted({M, _pad256(M)}):
        yield _gemm(prec, store, m, 3 * D, D, ks, xs)
        yield _gemm(prec, RESID, m, D, D, ks, xs)
        yield _gemm(prec, act, m, ff, D, ks, xs)
        yield _gemm(prec, RESID, m, D, ff, ks, xs)
    if cls:   # K and V of every token into the [M, 3 D] rows, then row 0 of every sequence: rows L tokens apart
        yield _gemm(prec, store, M, 2 * D, D, ks, xs, ldo=3 * D)
        yield _gemm(prec, store, nseq, D, D, ks, xs, ldx=L * D, ldo=3 * L * D)
        yield _gemm(prec, RESID, nseq, D, D, ks, xs, ldx=L * D, ldo=L * D)
        for m in sorted({nseq, _pad256(nseq)}):
            yield _gemm(prec, act, m, ff, D, ks, xs)
        yield _gemm(prec, RESID, nseq, D, ff, ks, xs, ldo=L * D)


def _groups():
    """{(kind, group name): [case line, ...]}: the sweep, the same for every CU count."""
    groups = {}
    for name, geo in GEOMETRIES.items():
        L, D, ff, erf = geo.v_tokens, geo.v_width, geo.v_mlp, geo.v_hidden_act == "gelu"
        kpad = (3 * geo.patch_size ** 2 + 63) // 64 * 64
        for form, prec, ks, xs in FORMS:
            cases = groups.setdefault(("gemm", f"{name} {form}"), [])
            for b in BATCHES:
                cases += _tower_gemms(prec, ks, xs, b, L, D, ff, erf, True)
                cases.append(_gemm(prec, PATCH, b * geo.n_patches, D, kpad, ks, xs))
                if not xs:
                    cases.append(_gemm(prec, PATCH, b * geo.n_patches, D, kpad, ks, 0, px=1))
                cases.append(f"Q {prec} {RESID} {_pad256(b * L)} {D}")
    for D, ff in sorted({(g.t_width, g.t_mlp) for g in GEOMETRIES.values()}):   # the text towers: 77 tokens per prompt
        for form, prec, ks, xs in FORMS[:5]:
            cases = groups.setdefault(("gemm", f"text-{D} {form}"), [])
            for k in (10, 100, 1000):
                cases += _tower_gemms(prec, ks, 0, k, 77, D, ff, False, False)
    for L in (1, 16, 50, 77, 197, 257, 288, 289, 577, 1025, 1026):
        for form, prec in (("bf16", BF16), ("fp16", F16), ("fp32", F32)):
            cases = groups.setdefault(("attn", f"L={L} {form}"), [])
            for hd, heads in ((64, 12), (80, 16)):
                for cus in CUS:   # nseq x heads on both sides of 16 x CUs (the persistent form's threshold)
                    for nseq in (16 * cus // heads, 16 * cus // heads + 1):
                        for qrows in (L, 1):
                            for causal in (0, 1):
                                for split in (0, 1):
                                    cases.append(f"T {prec} {nseq} {L} {heads} {hd} {causal} {qrows} 0 0 {split}")
    return groups


# ---- the labelled rows of the GPU tests ------------------------------------------------------------------------------------
def _assigned(path, name):
    """The value of the module-level `name = <literal arithmetic>` of a test file, read from its source (the GPU test modules
    need torch and a device to import)."""
    tree = ast.parse(open(os.path.join(ROOT, "tests", path)).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets):
            return eval(compile(ast.Expression(node.value), path, "eval"), {"__builtins__": {}})
    raise KeyError(name)


def _form(fid):
    """test_gpu_gelu.py FORMS by id: precision, then -W (split weights), -X (split activations), -OUT (split output)."""
    parts = fid.split("-")
    return PREC[parts[0]], int("W" in parts), int("X" in parts), "OUT" in parts


def _labelled():
    """[(label, expected family or None, case line)]: mcm_op_linear_ex launches these as given, no row padding."""
    rows = []
    large, small = _assigned("test_gpu_gelu.py", "LARGE"), _assigned("test_gpu_gelu.py", "SMALL")
    other = [("B16-b128-pingpong", 25600, 3072, 768), ("ragged-p256", 25216, 3072, 768)]   # ..._other_forms_within_budget
    src = open(os.path.join(ROOT, "tests", "test_gpu_gelu.py")).read()
    assert all(f'("{t}", {m}, {n}, {k})' in src for t, m, n, k in other)
    all_forms = ["bf16", "fp16", "fp32", "fp16-X", "fp16-X-OUT", "bf16-W", "fp16-W", "fp16-W-X-OUT"]
    assert all(f'"{f}"' in src for f in all_forms)
    for rows_of, forms in ((large, ["bf16", "fp16"]), (other, [f for f in all_forms if f not in ("bf16", "fp16")]),
                           (small, all_forms)):
        for tag, M, N, K in rows_of:
            for fid in forms:
                prec, ks, xs, outs = _form(fid)
                epi = GELU_ERF_X2 if outs else GELU_ERF
                rows.append((f"gelu {tag} {fid}", tag, _gemm(prec, epi, M, N, K, ks, xs)))
    for tag, M, shapes, _extra in _assigned("test_gpu_error_budget.py", "FULL"):
        for N, K, epi in shapes:   # what the comments above those rows say
            want = {"B32-b512": "sliver" if N == 768 else "pingpong", "text-K1000": "ragged-p256"}.get(tag)
            for fid in ("fp16", "bf16"):
                rows.append((f"budget {tag} N={N} K={K} epi={epi} {fid}", want, _gemm(PREC[fid], epi, M, N, K)))
    fp32_rows = "((25600, 768, 768, 2), (25600, 3072, 768, 1), (77000, 1536, 512, 0))"   # test_gemm_full_size_fp32_within_budget
    assert fp32_rows in open(os.path.join(ROOT, "tests", "test_gpu_error_budget.py")).read()
    for (M, N, K, epi), want in zip(eval(fp32_rows), ("sliver", "pingpong", "ragged-p256")):   # "... and the ragged text tower"
        rows.append((f"budget fp32 M={M} N={N} K={K} epi={epi}", want, _gemm(F32, epi, M, N, K)))
    for name, N, K, epi in _assigned("test_gpu_h14.py", "H14_GEMMS"):   # "65 792 rows = exactly 257 row tiles: the ping-pong kernel"
        rows.append((f"h14 {name} b256 fp16", "pingpong", _gemm(F16, (STORE, GELU_ERF, RESID)[epi], 65792, N, K)))
    return rows


def _family_ok(tag, launches):
    """Whether the launches of a labelled row are what its tag names."""
    kernels = [ln.split("<")[0].strip() for ln in launches]
    if tag is None:
        return True
    if tag == "sliver":   # cut at row 80 * 256: the ping-pong kernel above, a tile kernel below
        return len(kernels) == 2 and kernels[0] == "gemm_pp_kernel" and kernels[1] in ("gemm_tile_kernel", "gemm_tile64_kernel") \
            and " M=20480 " in launches[0]
    if "ragged-p256" in tag:
        return kernels == ["gemm_p256_kernel"]
    for kernel, word in FAMILY.items():
        if word in tag.split("-"):
            return kernels == [kernel]
    raise AssertionError(f"a tag this test cannot read: {tag}")


# ---- the recorder ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorder(tmp_path_factory):
    if not (os.path.isfile(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("launch_routes")
    procs = {}
    for which in ("GEMM", "ATTN"):
        exe = str(out / f"rec_{which.lower()}")
        procs[exe] = subprocess.Popen([HIPCC, "--offload-host-only", "-std=c++17", "-O1", "-w", "-I", os.path.join(ROOT, "mcm_amd", "csrc"),
                                       f"-DREC_{which}", os.path.join(ROOT, "tests", "launch_routes_rec.hip"), "-o", exe],
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    for exe, p in procs.items():
        log = p.communicate()[0]
        assert p.returncode == 0, log[-4000:]

    def run(kind, cus, cases):
        """[(case line, [launch line, ...], hipError_t)] of `cases` on `cus` CUs."""
        exe = str(out / ("rec_gemm" if kind == "gemm" else "rec_attn"))
        r = subprocess.run([exe, str(cus)], input="\n".join(cases) + "\n", capture_output=True, text=True, check=True)
        records, cur = [], None
        for line in r.stdout.splitlines():
            if line.startswith("  -> "):
                records.append((cur[0], cur[1], int(line[5:])))
            elif line.startswith("  "):
                cur[1].append(line.strip())
            else:
                cur = (line, [])
        assert [c for c, _, _ in records] == list(cases)
        return records

    return run


def _digest(records):
    fam = Counter()
    text = []
    for case, launches, err in records:
        text.append(case)
        text += launches
        text.append(str(err))
        for ln in launches:
            if "=" in ln.split()[0]:   # the answer of a Q line
                continue
            fam[ln.split("<")[0].split()[0]] += 1
    n_launch = sum(fam.values())
    refused = sum(1 for _, _, e in records if e)
    fams = " ".join(f"{k}={v}" for k, v in sorted(fam.items()))
    return f"cases={len(records)} launches={n_launch} refused={refused} {fams} sha={hashlib.sha256(chr(10).join(text).encode()).hexdigest()[:16]}"


@pytest.fixture(scope="module")
def routes(recorder, tmp_path_factory):
    """The text of the golden as this tree produces it, the labelled rows' records, and where the full records went."""
    lines = ["# tests/test_launch_routes_cpu.py; one line per launch: kernel grid block lds | the kernel's integer arguments",
             "# (GemmArgs: M N K gn and the byte offsets of x, out, resid from the pointers passed to launch_gemm)"]
    full = []
    labelled = []
    rows = _labelled()
    recs = recorder("gemm", 256, [c for _, _, c in rows])
    lines.append("[labelled rows of test_gpu_gelu.py, test_gpu_error_budget.py and test_gpu_h14.py, 256 CUs]")
    for (label, tag, _), (case, launches, err) in zip(rows, recs):
        labelled.append((label, tag, launches, err))
        lines.append(f"{label}: {case} -> {err}")
        lines += ["  " + ln for ln in launches]
    groups = _groups()
    shown = {("gemm", f"{n} fp16") for n in GEOMETRIES} | {("attn", f"L={L} fp16") for L in (50, 77, 197, 257, 577)}
    digests = []
    for cus in CUS:
        for (kind, name), cases in groups.items():
            recs = recorder(kind, cus, cases)
            full.append(f"[{cus} CUs] {kind} {name}")
            for case, launches, err in recs:
                full.append(f"{case} -> {err}")
                full += ["  " + ln for ln in launches]
            digests.append(f"cus={cus} {kind} {name}: {_digest(recs)}")
            if cus == 256 and (kind, name) in shown:
                lines.append(f"[256 CUs] {kind} {name}: the whole-batch layer at M padded to 256 rows" if kind == "gemm"
                             else f"[256 CUs] {kind} {name}: every query row, 64-wide heads")
                for case, launches, err in recs:
                    f = case.split()
                    keep = (f[0] == "G" and int(f[3]) % 256 == 0 and int(f[3]) > 4096 and f[2] != str(PATCH)) if kind == "gemm" else \
                        (f[5] == "64" and f[7] == f[3] and f[10] == "0" and int(f[2]) * int(f[4]) in (4092, 4104) and err == 0)
                    if keep:
                        lines.append(f"{case} -> {err}")
                        lines += ["  " + ln for ln in launches]
    lines.append("[digests: every group of the sweep on 256, 64 and 4 CUs]")
    lines += digests
    path = tmp_path_factory.mktemp("launch_routes_full") / "launch_routes_full.txt"
    path.write_text("\n".join(full) + "\n")
    return "\n".join(lines) + "\n", labelled, str(path)


def test_routes_match_the_golden(routes):
    text, _, full_path = routes
    if os.environ.get("MCM_WRITE_LAUNCH_ROUTES"):
        with open(GOLDEN, "w") as f:
            f.write(text)
    assert len(text) <= 100 * 1024
    want = open(GOLDEN).read()
    if text != want:
        got, exp = text.splitlines(), want.splitlines()
        diff = [f"line {i + 1}:\n  golden {e}\n  now    {g}" for i, (g, e) in enumerate(zip(got, exp)) if g != e][:10]
        pytest.fail(f"{len(got)} lines now, {len(exp)} in the golden; the full records of this run: {full_path}\n" + "\n".join(diff))


def test_labelled_rows_reach_the_family_their_tag_names(routes):
    """The tags of test_gpu_gelu.py LARGE / SMALL and the comments of test_gpu_error_budget.py FULL and test_gpu_h14.py are
    statements about routing on 256 CUs: checked here."""
    _, labelled, _ = routes
    assert len(labelled) > 60
    wrong = [(label, launches, err) for label, tag, launches, err in labelled if err != 0 or not _family_ok(tag, launches)]
    assert not wrong, wrong


def test_b32_batch_512_outproj_is_cut_at_the_sliver_round(recorder):
    """ViT-B/32 at batch 512, out-proj (M = 25600, N = 768): 300 tiles on 256 workgroups.  The ping-pong kernel takes the 80 row
    tiles of one whole round, the 64x128 tile kernel the other 20 on 480 workgroups."""
    (_, launches, err), = recorder("gemm", 256, [_gemm(F16, RESID, 25600, 768, 768)])
    assert err == 0 and len(launches) == 2
    assert re.match(r"gemm_pp_kernel<2, 2> grid=256,1,1 block=512 lds=\d+ \| M=20480 N=768 K=768 gn=3 x\+0 out\+-1 resid\+0$", launches[0])
    assert re.match(r"gemm_tile64_kernel<2, 2> grid=480,1,1 block=256 lds=\d+ \| M=5120 N=768 K=768 gn=3 x\+31457280 out\+-1 "
                    r"resid\+62914560$", launches[1])

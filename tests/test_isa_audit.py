"""The compiler's gfx950 output of every kernel file that places its own s_barrier, audited on the CPU.

Rule (the wrong tile of round 5): an LDS read is waited for before the barrier that hands
its source to the next writer.  `tools/audit_barriers.py` walks the basic blocks of the listing with the
LGKM queue as its state and reports every barrier that can be reached with a ds_read in flight.

What is audited.  The set is computed: every `csrc/*.hip` whose text names `s_barrier` or
`__builtin_amdgcn_s_barrier` (today the persistent 3x3 kernel, the deformable team form and the deformable
wide form), plus the offset convolution and the 1x1 projection, whose only barriers are __syncthreads, as
explicit extras.  A new kernel file with a raw barrier is audited without anybody adding it here.  Every
listing is compiled with the command line `csrc/Makefile` gives that file (`make -n`), so per-file flags --
`-fno-slp-vectorize` for cn_dcn4 -- are the shipped ones.

What is held.  Every shipped instantiation (DBG = false) of every audited kernel has ZERO UNEXPLAINED
reports.  All but `dcn_wide_kernel` have zero reports.  The wide form places its per-step barrier with
team 0's next request deliberately in flight (cn_dcn4.hip, the step loop's schedule): each of its reports
is recorded in WIDE_EXPECTED by template arguments with a signature -- which reads (count, width, immediate
offset), whether they arrive round a back-edge, which KINDS of LDS writer follow up to the next barrier --
and the reason why those writers cannot touch what is read.  A report that is not in the table, a recorded
one that is gone, other reads, or a ds_write behind such a barrier fails the test and prints the listing
lines.

Exempt by name: the probe instantiations `conv3x3p_kernel<., ., DBG = true, ...>` and
`dcn_wide_kernel<., ., DBG = true>`.  Their switchable paths (cn_set_tuning key 9: no barrier, no MFMAs,
no sampling ...) are infeasible combinations to a path-insensitive walk, some of them unsafe on purpose,
and nothing launches them outside `tools/bench_c3p.py PROBE=1` / a key 9 probe run.
"""
import glob
import importlib.util
import os
import re
import shlex
import shutil
import subprocess
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "centernet_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
EXTRA_FILES = ["cn_offconv", "cn_proj"]     # __syncthreads only: audited all the same


def audited_files(csrc=CSRC):
    """every kernel file that places a raw barrier, by its text, and the explicit extras"""
    raw = []
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        with open(path) as f:
            text = f.read()
        if "s_barrier" in text:              # covers __builtin_amdgcn_s_barrier and inline assembly
            raw.append(os.path.splitext(os.path.basename(path))[0])
    return raw + [n for n in EXTRA_FILES if n not in raw]


def _tool():
    spec = importlib.util.spec_from_file_location("audit_barriers", os.path.join(ROOT, "tools", "audit_barriers.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def makefile_command(name):
    """argv of the compile step csrc/Makefile runs for <name>.o (`make -n`: nothing is built)"""
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, "OBJDIR=.", "HIPCC=" + HIPCC, name + ".o"],
                         check=True, capture_output=True, text=True).stdout
    cmds = [shlex.split(l) for l in out.splitlines() if name + ".hip" in l and " -c " in l]
    assert len(cmds) == 1, out
    return cmds[0]


def _listing(name, out_dir):
    """the device listing of the shipped object: the Makefile's command with -c / -o replaced"""
    argv = makefile_command(name)
    i = argv.index("-o")
    argv = [a for k, a in enumerate(argv) if k not in (i, i + 1) and a != "-c"]
    out = os.path.join(out_dir, name + ".s")
    subprocess.run(argv + ["-S", "--cuda-device-only", "-o", out], check=True, capture_output=True, cwd=CSRC)
    return out


# ---- dcn_wide_kernel<NB, MSIG, DBG>: the reports that are expected, and why each is safe ----------------------
# reads of one request() of cn_dcn4.hip:255-289: four corner pairs of the window being sampled (quad and
# quad ^ 16 of the pixels at +0 and one window row down, +DCNW_ROWB = 3072) ...
_WINDOW = {("ds_read_b128", 0): 4, ("ds_read_b128", 3072): 4}
# ... behind the record of the NEXT step (record(), :251-252): corner weights at DCNW_RECW = 49152 + step * 2048
# (float4 [9][128]) and the two swizzled offsets (uint2, DCNW_RECP folded into the address register)
_STEP_READS = {**_WINDOW, ("ds_read_b128", 49152): 1, ("ds_read_b64", 0): 1}
# the same request seen through the loop's back-edge: the record address is a running pointer there
_EXIT_READS = {**_WINDOW, ("ds_read_b128", 2048): 1, ("ds_read_b64", 0): 1}

STEP_BARRIER = dict(
    reads=_STEP_READS, back_edge=False, writers=["dma"],
    reason="""dcnw_barrier of step t >= 1 (cn_dcn4.hip:359).  In flight BY DESIGN (:234-244): team 0's request for step
t + 1, issued at the end of step t - 1 behind the MFMAs (:422) and blended at the end of step t (:420) -- the
record of step t + 2 in [DCNW_RECW, W_EPI) (:251-252) and eight reads of the window being sampled,
[wbase, wbase + DCNW_WBYTES) (:281-288).  Every LDS writer up to the next barrier is LDS-DMA: dma_w1 into ring
slot (step + 1) & 1, at W_RING and above (:142-149, :385), and for NB = 4 one piece of the NEXT chunk's window
into wbase ^ W_WIN1 (:379, :381), the window that is NOT being sampled.  Records are written in the prologue
only (:215-216).  No writer shares a region with a read; a ds_write here would void the argument.""")
SWAP_BARRIER = dict(
    reads=_EXIT_READS, back_edge=True, writers=["dma"],
    reason="""__syncthreads of the window swap (cn_dcn4.hip:329), entered from the step loop's exit.  The walk carries
team 0's request(t + 2) (:422) round the loop's back-edge and straight out of the loop -- a path no wave takes:
the request is issued only while t < 7 and the loop leaves only after t = 8 (:352).  Steps t = 7 and t = 8 each
wait lgkmcnt(0) for their ring fragments in front of the first MFMA (:400, in-order return retires everything
older) and issue no request behind it (team 0: none at t = 7 / 8, :422; team 1: none at t = 8, :365).  So no
record or window read is outstanding at :329, and the DMA that follows through the barrier-less step 0 (:379 /
:381 into wbase ^ W_WIN1, after :330 the window just left; :385 into the ring) cannot overtake one.""")

WIDE_EXPECTED = {
    # (NB, MSIG, DBG): reports in listing order
    (8, True, False): [STEP_BARRIER],
    (8, False, False): [STEP_BARRIER],
    (4, True, False): [SWAP_BARRIER, STEP_BARRIER],
    (4, False, False): [SWAP_BARRIER, STEP_BARRIER],
}
WIDE_PROBES = {(8, True, True), (4, True, True)}      # exempt by name, see the module text


def _demangle(mangled):
    if not shutil.which("c++filt"):
        return mangled
    return subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()


def _template_args(name, kernel):
    m = re.search(re.escape(kernel) + r"<([^>]*)>", name)
    if not m:
        return None
    conv = {"true": True, "false": False}
    return tuple(conv[a.strip()] if a.strip() in conv else int(a.strip()) if a.strip().lstrip("-").isdigit() else a.strip()
                 for a in m.group(1).split(","))


def check_reports(name, reports, expected):
    """`reports` (tool.flagged) of one kernel against its recorded signatures: None, or what is wrong"""
    wrong = []
    if len(reports) != len(expected):
        wrong.append("%d barriers flagged, %d recorded" % (len(reports), len(expected)))
    for k, rep in enumerate(reports):
        exp = expected[k] if k < len(expected) else None
        why = []
        if exp is None:
            why.append("not recorded")
        else:
            if Counter(rep["reads"]) != Counter(exp["reads"]):
                why.append("reads in flight %r, recorded %r" % (sorted(Counter(rep["reads"]).items()), sorted(exp["reads"].items())))
            if rep["back_edge"] != exp["back_edge"]:
                why.append("back-edge %r, recorded %r" % (rep["back_edge"], exp["back_edge"]))
            if rep["writers"] != exp["writers"]:
                why.append("LDS writers up to the next barrier %r, recorded %r" % (rep["writers"], exp["writers"]))
        if why:
            wrong.append("barrier at line %d: %s\n%s" % (rep["line"], "; ".join(why), "\n".join(rep["text"])))
    return ("%s:\n%s" % (name, "\n".join(wrong))) if wrong else None


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not present")
def test_no_lds_read_in_flight_at_a_barrier(tmp_path):
    tool = _tool()
    files = audited_files()
    assert {"cn_conv3x3p", "cn_dcn3", "cn_dcn4", "cn_offconv", "cn_proj"} <= set(files)
    # the audited listing is the shipped code: the per-file flag of cn_dcn4 comes through
    assert "-fno-slp-vectorize" in makefile_command("cn_dcn4")
    assert "-fno-slp-vectorize" not in makefile_command("cn_dcn3")
    with ThreadPoolExecutor(len(files)) as ex:
        listings = list(ex.map(lambda n: _listing(n, str(tmp_path)), files))
    seen = 0
    wide_seen, proj_seen = set(), set()
    failures = []
    for path in listings:
        res = tool.flagged(path)
        assert res, path
        counts = tool.audit(path)
        for mangled, reports in res.items():
            assert counts[mangled][1] == len(reports)
            name = _demangle(mangled)
            args = _template_args(name, "conv3x3p_kernel")
            if args is not None and args[2] is True:          # DBG
                continue
            args = _template_args(name, "dcn_wide_kernel")
            expected = []
            if args is not None:
                wide_seen.add(args)
                if args in WIDE_PROBES:
                    continue
                assert args[2] is False, name
                expected = WIDE_EXPECTED.get(args, [])
            if _template_args(name, "proj1x1_kernel") is not None:
                proj_seen.add(_template_args(name, "proj1x1_kernel"))
            seen += 1
            bad = check_reports(name, reports, expected)
            if bad:
                failures.append(bad)
    assert not failures, "\n\n".join(failures)
    assert seen >= 20 + len(WIDE_EXPECTED) + 4
    assert wide_seen == set(WIDE_EXPECTED) | WIDE_PROBES, wide_seen
    assert proj_seen == {(True, 2), (True, 4), (False, 2), (False, 4)}, proj_seen
    for sig in (STEP_BARRIER, SWAP_BARRIER):
        assert sig["writers"] == ["dma"] and len(sig["reason"]) > 200 and "cn_dcn4.hip" in sig["reason"]


def test_every_recorded_report_is_needed_and_any_other_fails():
    """the comparison itself: an entry taken out of the table, a report with other reads and a ds_write
    behind a recorded barrier each fail"""
    rep = dict(line=10, reads=[k for k, n in _STEP_READS.items() for _ in range(n)], back_edge=False,
               writers=["dma"], text=["    10  s_barrier"])
    assert check_reports("k", [rep], [STEP_BARRIER]) is None
    assert "1 barriers flagged, 0 recorded" in check_reports("k", [rep], [])
    assert "0 barriers flagged, 1 recorded" in check_reports("k", [], [STEP_BARRIER])
    assert "reads in flight" in check_reports("k", [dict(rep, reads=rep["reads"][:-1])], [STEP_BARRIER])
    assert "reads in flight" in check_reports("k", [dict(rep, reads=rep["reads"] + [("ds_read_b128", 79872)])], [STEP_BARRIER])
    assert "LDS writers" in check_reports("k", [dict(rep, writers=["dma", "ds_write"])], [STEP_BARRIER])
    assert "back-edge" in check_reports("k", [dict(rep, back_edge=True)], [STEP_BARRIER])
    assert "s_barrier" in check_reports("k", [dict(rep, writers=[])], [STEP_BARRIER])      # the listing lines are printed


def test_the_audited_set_is_computed_from_the_sources(tmp_path):
    """a new kernel file with a raw barrier joins the audit by itself"""
    for n in ("cn_a", "cn_b", "cn_c"):
        (tmp_path / (n + ".hip")).write_text({"cn_a": "__global__ void k() { __syncthreads(); }\n",
                                              "cn_b": "__global__ void k() { __builtin_amdgcn_s_barrier(); }\n",
                                              "cn_c": '__global__ void k() { asm volatile("s_barrier"); }\n'}[n])
    assert audited_files(str(tmp_path)) == ["cn_b", "cn_c"] + EXTRA_FILES
    assert audited_files()[:3] == ["cn_conv3x3p", "cn_dcn3", "cn_dcn4"]


def test_the_walk_sees_a_read_across_a_barrier(tmp_path):
    """the tool itself: a read that is waited for, one that is not, one behind a join"""
    tool = _tool()
    src = """
_Z1kv:
	ds_read_b128 v[0:3], v8
	s_waitcnt lgkmcnt(0)
	s_barrier
	ds_read_b128 v[4:7], v8
	s_cbranch_scc1 .LBB0_2
	s_waitcnt lgkmcnt(0)
.LBB0_2:
	s_barrier
	ds_write_b32 v8, v4
	s_waitcnt lgkmcnt(0)
	ds_read_b32 v9, v8
	ds_read_b32 v10, v8 offset:4
	s_waitcnt lgkmcnt(1)
	s_barrier
	s_endpgm
.Lfunc_end0:
"""
    p = tmp_path / "k.s"
    p.write_text(src)
    assert tool.audit(str(p)) == {"_Z1kv": (3, 2)}
    rep = tool.flagged(str(p))["_Z1kv"]
    assert [(r["line"], r["reads"], r["back_edge"], r["writers"]) for r in rep] == [
        (10, [("ds_read_b128", 0)], False, ["ds_write"]),
        (16, [("ds_read_b32", 4)], False, [])]


def test_the_report_names_reads_behind_a_back_edge_and_the_writers_on_every_path(tmp_path):
    """flagged(): a read carried round a loop back-edge into the barrier at the loop's head (the shape of the
    wide form's window swap), writers found through an iteration that branches round its own barrier, and a
    kernel without a flagged barrier"""
    tool = _tool()
    src = """
_Z5outerv:
	s_waitcnt lgkmcnt(0)
.LBB0_1:
	s_barrier
	s_cbranch_scc1 .LBB0_3
	global_load_lds_dwordx4 v[0:1], off
.LBB0_3:
	ds_read_b128 v[4:7], v8 offset:2048
	ds_read_b64 v[2:3], v9
	s_cbranch_scc0 .LBB0_1
	s_waitcnt lgkmcnt(0)
	s_barrier
	ds_write_b32 v8, v4
	s_endpgm
.Lfunc_end0:
_Z5innerv:
	ds_read_b128 v[0:3], v8 offset:49152
	s_barrier
	s_waitcnt lgkmcnt(0)
.LBB1_1:
	s_cbranch_scc1 .LBB1_2
	s_barrier
.LBB1_2:
	buffer_load_dword v1, s[0:3], 0 offen lds
	s_waitcnt lgkmcnt(0)
	s_cbranch_scc0 .LBB1_1
	s_barrier
	ds_write_b64 v8, v[4:5]
	s_endpgm
.Lfunc_end1:
_Z5cleanv:
	ds_read_b32 v0, v8
	s_waitcnt lgkmcnt(0)
	s_barrier
	ds_write_b32 v8, v0
	s_endpgm
.Lfunc_end2:
"""
    p = tmp_path / "k.s"
    p.write_text(src)
    rep = tool.flagged(str(p))
    assert tool.audit(str(p)) == {"_Z5outerv": (2, 1), "_Z5innerv": (3, 1), "_Z5cleanv": (1, 0)}
    assert rep["_Z5cleanv"] == []
    (o,), (i,) = rep["_Z5outerv"], rep["_Z5innerv"]
    assert (o["line"], o["reads"], o["back_edge"], o["writers"]) == (5, [("ds_read_b128", 2048), ("ds_read_b64", 0)], True, ["dma"])
    assert any("behind a back-edge" in l for l in o["text"])
    # the first trip of the loop skips its barrier: the DMA behind it still follows the flagged barrier; the
    # ds_write behind the LAST barrier does not
    assert (i["line"], i["reads"], i["back_edge"], i["writers"]) == (19, [("ds_read_b128", 49152)], False, ["dma"])

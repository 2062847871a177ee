"""What the F5 tests (tests/test_f5_*.py) share: a scenario as a realignment job, the job through one of the three chains -- the
host path (enumeration = 0), the staged chain ($SK_A5_FUSED=0) and F5 -- with everything the tests compare, and the child processes
of the tests whose switches are read once per process.  A plain module: the scenario builders stay with their tests."""
import ctypes as C
import os
import subprocess
import sys

from strelka_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_job(sc, enumeration):
    job = capi.RealignJob(capi.realign_options(is_haplotyping_enabled=sc["is_haplotyping_enabled"],
                                               min_read_bp_flank=sc["min_read_bp_flank"], enumeration=enumeration))
    job.set_reference(sc["ref_seq"], sc["ref_offset"])
    job.set_indels(sc["indels"])
    return job


def add_reads(job, reads):
    """the job's index of every read, None for one the gate turns down"""
    idx = []
    for rd in reads:
        try:
            idx.append(job.add_read(rd["code"], rd["qual"], rd["pos"], rd["path"], rd["is_fwd"], rd["map_level"], 0, rd["realign_range"],
                                    rd["observed"]))
        except capi.StrelkaAmdError:
            idx.append(None)
    return idx


def run_chain(sc, chain, reads=None, *, one_wait="1", rescore=0, setenv=os.environ.__setitem__):
    """the scenario's reads (or `reads`) as one job through chain "host", "staged" or "f5"; rescore: sk_realign_job_rescore with that many
    repeats between the run and the reading of the results.  setenv: monkeypatch.setenv in a test, os.environ in a child process.
    res: repr of every result (None for a read the gate turned down), got: the results, idx: the reads' indices; what the process's
    counters moved by over the job: reference reads outside, jobs (one wait, run again, staged), launches of the table kernel, rounds
    scored by a helper"""
    setenv("SK_A5_FUSED", "0" if chain == "staged" else "1")
    setenv("SK_ENUM_ONE_WAIT", one_wait)
    before = capi.RealignJob.device_job_counts()
    launches0 = capi.RealignJob.f5_tail_launches()
    shared0 = capi.RealignJob.f5_shared_rounds()
    outside0 = capi.lib().sk_realign_reference_reads_outside()
    job = make_job(sc, 0 if chain == "host" else 2)
    idx = add_reads(job, sc["reads"] if reads is None else reads)
    job.run()
    if rescore:
        ms, nr, nc, cells = C.c_float(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
        assert capi.lib().sk_realign_job_rescore(rescore, C.byref(ms), C.byref(nr), C.byref(nc), C.byref(cells)) == 0, capi.last_error()
    got = [None if i is None else job.result(i) for i in idx]
    return dict(res=[None if x is None else repr(x) for x in got], got=got, idx=idx, consulted=job.indels_consulted().tolist(),
                outside=capi.lib().sk_realign_reference_reads_outside() - outside0, counts=job.enumeration_counts(),
                jobs=tuple(b - a for a, b in zip(before, capi.RealignJob.device_job_counts())),
                launches=capi.RealignJob.f5_tail_launches() - launches0, shared=capi.RealignJob.f5_shared_rounds() - shared0)


def assert_same(a, b, what):
    assert a["res"] == b["res"], what
    assert a["consulted"] == b["consulted"], what
    assert a["outside"] == b["outside"], what


def fresh_f5(sc, reads, **kw):
    """an F5 job that does not follow a job of its own layout: the scores are not cleared between jobs, and after an identical job
    a read that a hand-out skipped, or a round nobody scored, would still find its right scores there -- so the same reads in reverse
    order go first.  (shared: the helped rounds of both jobs; everything else is the second job's)"""
    first = run_chain(sc, "f5", reads[::-1])
    out = run_chain(sc, "f5", reads, **kw)
    out["shared"] += first["shared"]
    return out


def spawn_child(file, mode, form, ok_token, timeout=300, **env):
    """`python <file> <mode> <form>` with the switches of `env` set (None: unset) -- they are read once per process.  The child's output,
    after the checks that it ended well and printed ok_token"""
    child_env = dict(os.environ)
    for k, v in env.items():
        child_env.pop(k, None)
        if v is not None:
            child_env[k] = str(v)
    p = subprocess.run([sys.executable, os.path.abspath(file), mode, str(form)], env=child_env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=timeout)
    out = p.stdout.decode(errors="replace")
    print(out[-3000:])
    assert p.returncode == 0 and ok_token in out, out[-3000:]
    return out

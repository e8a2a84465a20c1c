"""The twelve-wave HF + PS kernel (k_hfps12, profiles/r04_experiments.md E1) is not shipped -- it is slower -- but it is
kept buildable (`tools/build_variants.sh tuning "-DHEAAC_TUNING"` -> ab/libtuning.so, launched with HEAAC_HFPS12=1), and
what is kept is kept correct: the HE-AACv2 parity tests run against it in a child process.  The variant is not part of
build(), so the test builds it itself from today's sources, into its own temporary directory."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_variant(tmp):
    """tools/build_variants.sh tuning "-DHEAAC_TUNING", into `tmp`: the sources are copied so that the product's
    objects under csrc/_obj are neither used nor touched."""
    import glob
    import shutil
    csrc = os.path.join(ROOT, "ffmpeg-heaac_amd", "csrc")
    work = os.path.join(tmp, "csrc")
    os.makedirs(work)
    for f in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.[ch]")) + [os.path.join(csrc, "Makefile")]:
        shutil.copy(f, work)
    lib = os.path.join(tmp, "libtuning.so")
    jobs = str(min(16, int(os.environ.get("MAX_JOBS") or 8)))
    subprocess.check_call(["make", "-C", work, "-j" + jobs, "-s", "ROOT=" + ROOT, "EXTRA=-DHEAAC_TUNING", "OUT=" + lib])
    return lib


@pytest.mark.gpu
def test_twelve_wave_variant_is_bit_exact(tmp_path):
    LIB = _build_variant(str(tmp_path))
    env = dict(os.environ, HEAAC_LIB_PATH=LIB, HEAAC_HFPS12="1")
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_he_gpu.py"),
                        os.path.join(ROOT, "tests", "test_golden.py"), "-m", "gpu", "-x", "-q", "-k", "hev2 or unstored or golden or codec"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1200)
    tail = "\n".join(p.stdout.splitlines()[-15:])
    assert p.returncode == 0, tail
    assert " passed" in tail, tail
    # (and the child really ran on the variant library)
    q = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import __graft_entry__ as g; "
                        "p = g.load_package(); print(p.LIB_OVERRIDDEN, p.LIB_PATH)" % ROOT],
                       env=env, stdout=subprocess.PIPE, text=True, timeout=300)
    assert q.stdout.split()[:2] == ["True", LIB], q.stdout

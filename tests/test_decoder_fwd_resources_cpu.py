"""Register budget of the kernels that share the decoder forward piece of csrc/vae_dev.hpp (dec_fwd_carve, decoder_fwd_stage,
decoder_fwd_layers, decoder_fwd_rows): k_decoder_fwd (vae_mnist.hip), k_generate (generate.hip), k_casale_generate
(casale_generate.hip).  k_decoder_fwd sits at 252 / 254 of the 256 VGPRs its launch bound of 512 threads allows, and a spill shows
in no result, only in time.  So the compiler's own resource remarks are checked: no scratch in any kernel of the three files, and
the six instances of the shared piece within 256 VGPRs."""
import os
import re
import shutil
import subprocess
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svgp-vae_amd", "csrc")
FILES = ("vae_mnist", "generate", "casale_generate")
# mangled names: <length><name>ILb<0|1>EE
SHARED = [f"{len(k)}{k}ILb{i}EE" for k in ("k_decoder_fwd", "k_generate", "k_casale_generate") for i in (0, 1)]


def resource_remarks(stderr):
    """{mangled kernel name: dict(vgprs, scratch)} of a -Rpass-analysis=kernel-resource-usage compile."""
    kernels, name = {}, None
    for line in stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                kernels[name][key] = int(m.group(1))
    return kernels


def test_decoder_forward_kernels_compile_without_scratch_within_256_vgprs():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as d:
        procs = [subprocess.Popen([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function",
                                   "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, f + ".hip"), "-o",
                                   os.path.join(d, f + ".o")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for f in FILES]
        outs = [p.communicate() for p in procs]
    kernels = {}
    for f, p, (_, err) in zip(FILES, procs, outs):
        assert p.returncode == 0, (f, err[-2000:])
        kernels.update(resource_remarks(err))
    shared = {s: [k for k in kernels if s in k] for s in SHARED}
    assert all(len(v) == 1 for v in shared.values()), shared
    for k, v in sorted(kernels.items()):
        print(f"{k}: {v['vgprs']} VGPRs, scratch {v['scratch']}")
        assert v["scratch"] == 0, (k, v)
    for (k,) in shared.values():
        assert kernels[k]["vgprs"] <= 256, (k, kernels[k])

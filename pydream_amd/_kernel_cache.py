"""Compiling a likelihood's source once: the hipcc / host-compiler runs behind pydream_amd.likelihoods and the cache of what they made."""
import hashlib
import os
import stat
import subprocess
import tempfile
import threading

_COMPILER_VERSION = {}
_FALLBACK_DIR = []


def _hipcc():
    return next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), "hipcc")


def _compiler_version(cc):
    """`cc --version` (memoised per process), part of the cache key: an object is only as current as the compiler that made it."""
    if cc not in _COMPILER_VERSION:
        try:
            _COMPILER_VERSION[cc] = subprocess.run([cc, "--version"], capture_output=True, text=True).stdout
        except OSError:
            _COMPILER_VERSION[cc] = ""
    return _COMPILER_VERSION[cc]


def _private_dir(path):
    """path is a directory (not a link) owned by this user and writable by nobody else."""
    try:
        st = os.lstat(path)
    except OSError:
        return False
    return stat.S_ISDIR(st.st_mode) and st.st_uid == os.getuid() and not (st.st_mode & (stat.S_IWGRP | stat.S_IWOTH))


def kernel_cache_dir():
    """Where compiled likelihood objects are kept: $DREAMZS_KERNEL_CACHE (default ~/.cache/dreamzs_kernels) if it can be written, else
    <tmpdir>/dreamzs_kernels_<uid>.  The last one has a predictable name in a shared directory, so it is created with mode 0700 and
    used only while it is a directory owned by this user and not group- or world-writable; otherwise a fresh private directory
    (mkdtemp) serves this process.  Objects found in the cache are loaded and run, so nobody else may be able to write there."""
    cdir = os.environ.get("DREAMZS_KERNEL_CACHE") or os.path.join(os.path.expanduser("~"), ".cache", "dreamzs_kernels")
    try:
        os.makedirs(cdir, exist_ok=True)
        if not os.access(cdir, os.W_OK):
            raise OSError("not writable")
        return cdir
    except OSError:
        pass
    cdir = os.path.join(tempfile.gettempdir(), "dreamzs_kernels_%d" % os.getuid())
    try:
        os.mkdir(cdir, 0o700)
    except OSError:
        pass
    if _private_dir(cdir):
        return cdir
    if not _FALLBACK_DIR or not _private_dir(_FALLBACK_DIR[0]):
        _FALLBACK_DIR[:] = [tempfile.mkdtemp(prefix="dreamzs_kernels_")]
    return _FALLBACK_DIR[0]


def _build_cached(text, suffix, src_ext, cmd_for, what, cached_key_parts, out_path=None):
    # what: (the compiler's name, what it was building) for the error messages
    """Compile `text` with the command cmd_for(src, out) into out_path or, without one, into the kernel cache under a key of
    (cached_key_parts, text).  Built beside the target under a name unique to the process and thread, then renamed into place:
    concurrent builders never see half a file."""
    cached = out_path is None
    if cached:
        key = hashlib.sha256(("\0".join(cached_key_parts) + "\0" + text).encode()).hexdigest()[:32]
        out_path = os.path.join(kernel_cache_dir(), key + suffix)
        if os.path.exists(out_path) and os.path.getsize(out_path) > 0:
            return out_path
    tmp = "%s.%d.%d.tmp" % (out_path, os.getpid(), threading.get_ident())
    src = tmp + src_ext
    with open(src, "w") as f:
        f.write(text)
    cmd = cmd_for(src, tmp)
    try:
        res = subprocess.run(cmd, capture_output=True, text=True)
    except OSError as ex:          # (no compiler on this machine: say so -- a code object built elsewhere can be given by path)
        os.remove(src)
        raise Exception("%s failed%s: cannot run %r (%s); set HIPCC, or build the code object where ROCm is installed and pass its path" % (what + (cmd[0], ex)))
    try:
        os.remove(src) if cached else os.replace(src, out_path + src_ext)
    except OSError:
        pass
    if res.returncode != 0:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise Exception("%s failed%s:\n%s" % (what + (res.stderr[-4000:],)))
    os.replace(tmp, out_path)
    return out_path


def compile_device_kernel(source, out_path=None, extra_flags=(), arch="gfx950"):
    """HIP source text -> a code object (.hsaco) for DeviceKernelLogLike: `hipcc --offload-arch=<arch> --genco` (arch: the engine is built
    for gfx950, the MI355X; the argument is there so that an error names what was asked for).
    -ffp-contract=off is on by default so that a density written with + and * rounds like the same expression in numpy (a host
    likelihood and its device twin then make the same accept / reject decisions bit for bit); pass extra_flags=("-ffp-contract=fast",)
    to let the compiler fuse.  Without out_path the code object is CACHED under a key of (source, flags, arch, `hipcc --version`) in
    kernel_cache_dir(): the same source is compiled once, by whichever process or unpickled copy asks first (advisor, round 5: a fresh
    temporary directory and a fresh hipcc run per call).  Returns the path."""
    text = source if "hip_runtime.h" in source else "#include <hip/hip_runtime.h>\n" + source
    flags = ["--offload-arch=%s" % arch, "--genco", "--no-gpu-bundle-output", "-O3", "-std=c++17", "-ffp-contract=off"] + list(extra_flags)
    hipcc = _hipcc()
    key = flags + ([_compiler_version(hipcc)] if out_path is None else [])
    return _build_cached(text, ".hsaco", ".hip", lambda src, out: [hipcc] + flags + ["-o", out, src],
                         ("hipcc", " for the device likelihood (--offload-arch=%s)" % arch), key, out_path)


def csrc_dir():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")

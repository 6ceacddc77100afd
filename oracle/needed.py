"""Make oracle/_ref/adapter_check load libmulls_hip.so by name, wherever its oracle/_ref/ was built.

A binary linked against a library without SONAME by path records that path in its DT_NEEDED entry, and the loader then opens exactly that
path: the binary works only in the checkout it was linked in.  oracle/build_ref.sh links by name, but it needs the reference sources, so an
oracle/_ref/ built elsewhere (or by an older recipe) is used as it is.  by_name() turns such a path entry into the bare file name; the binary's
RUNPATH ($ORIGIN/../../mulls_amd) then finds the library of the checkout it sits in.  The path entry ends in the file name, so the string table
already holds it as a suffix: only the entry's offset into the string table changes, no string and no size.

    python -m oracle.needed oracle/_ref/adapter_check
"""
import os
import struct
import sys

LIB = "libmulls_hip.so"
PT_LOAD, PT_DYNAMIC = 1, 2
DT_NULL, DT_NEEDED, DT_STRTAB = 0, 1, 5


def _needed(data):
    """[(file offset of the DT_NEEDED entry's value, string-table file offset of its name)] of a little-endian ELF64 file."""
    if data[:4] != b"\x7fELF" or data[4] != 2 or data[5] != 1:
        raise ValueError("not a little-endian ELF64 file")
    phoff, = struct.unpack_from("<Q", data, 0x20)
    phentsize, phnum = struct.unpack_from("<HH", data, 0x36)
    loads, dyn = [], None
    for i in range(phnum):
        p_type, _, p_offset, p_vaddr, _, p_filesz = struct.unpack_from("<IIQQQQ", data, phoff + i * phentsize)
        if p_type == PT_LOAD:
            loads.append((p_vaddr, p_offset, p_filesz))
        elif p_type == PT_DYNAMIC:
            dyn = (p_offset, p_filesz)
    if dyn is None:
        return []
    entries, strtab = [], None
    for off in range(dyn[0], dyn[0] + dyn[1], 16):
        tag, val = struct.unpack_from("<qQ", data, off)
        if tag == DT_NULL:
            break
        if tag == DT_NEEDED:
            entries.append((off + 8, val))
        elif tag == DT_STRTAB:
            strtab = val
    base = next((o + strtab - v for v, o, n in loads if strtab is not None and v <= strtab < v + n), None)
    if base is None:
        raise ValueError("string table outside the loaded segments")
    return [(voff, base + val) for voff, val in entries]


def by_name(path, lib=LIB):
    """Rewrite a DT_NEEDED entry of `path` that names `lib` by a path to the bare name (atomically: a new file replaces the old one).
    Returns True if the file changed."""
    with open(path, "rb") as f:
        data = bytearray(f.read())
    changed = False
    for voff, soff in _needed(data):
        name = bytes(data[soff:data.index(b"\0", soff)]).decode()
        if name != lib and os.path.basename(name) == lib:
            val, = struct.unpack_from("<Q", data, voff)
            struct.pack_into("<Q", data, voff, val + len(name) - len(lib))
            changed = True
    if changed:
        tmp = path + ".tmp"
        try:
            with open(tmp, "wb") as f:
                f.write(data)
            os.chmod(tmp, os.stat(path).st_mode & 0o7777)
            os.replace(tmp, path)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    return changed


if __name__ == "__main__":
    for p in sys.argv[1:]:
        print("%s: %s" % (p, "now loads %s by name" % LIB if by_name(p) else "unchanged"))

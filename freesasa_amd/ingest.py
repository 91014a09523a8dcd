"""Python face of include/freesasa_ingest.h: multi-threaded PDB / mmCIF -> packed batch.

    batch = ingest.load_pdb_files(paths)            # host threads, one structure per file
    sasa, totals = freesasa_amd.calc_batch(batch.xyz, batch.radii, batch.offsets)
    per_res = batch.residue_sums(sasa)              # or GpuContext.segment_sums on the device

What a file contributes is what the reference's freesasa_structure_from_pdb() holds for it
(ref: src/structure.c:644-722); the parsing itself is C (freesasa_amd/csrc/ingest.c)."""
import ctypes as C

import numpy as np

from . import lib

INCLUDE_HETATM, INCLUDE_HYDROGEN, JOIN_MODELS = 1, 1 << 2, 1 << 5     # ref: src/freesasa.h:182-191
HALT_AT_UNKNOWN, SKIP_UNKNOWN, RADIUS_FROM_OCCUPANCY = 1 << 6, 1 << 7, 1 << 8
PARSE_ON_DEVICE = 1 << 16       # sweep drivers only: the files' text is parsed by kernels (csrc/gpu_parse.hip)
OK, EIO, EFORMAT, EEMPTY, EUNKNOWN, EOPTION, ENOMEM, EVERSION, EGROUP = range(9)
GROUPS_LONG, SEPARATE_CHAINS = 1, 1 << 4   # flags of freesasa_ingest_chain_groups
APOLAR, POLAR, UNKNOWN = 0, 1, 2


class _CBatch(C.Structure):
    _fields_ = [("n_structs", C.c_int32), ("n_atoms", C.c_int64), ("n_residues", C.c_int64),
                ("xyz", C.POINTER(C.c_double)), ("radii", C.POINTER(C.c_double)),
                ("atom_class", C.POINTER(C.c_uint8)), ("atom_backbone", C.POINTER(C.c_uint8)),
                ("atom_name", C.POINTER(C.c_char)), ("atom_symbol", C.POINTER(C.c_char)),
                ("offsets", C.POINTER(C.c_int64)),
                ("res_first", C.POINTER(C.c_int64)), ("res_offsets", C.POINTER(C.c_int64)),
                ("res_ref", C.POINTER(C.c_int16)), ("res_name", C.POINTER(C.c_char)), ("res_number", C.POINTER(C.c_char)),
                ("res_chain", C.POINTER(C.c_char)), ("status", C.POINTER(C.c_int32))]


def _arr(ptr, n, dtype):
    """numpy copy of n items behind a ctypes pointer (one memcpy; np.ctypeslib.as_array is slow on large arrays)"""
    if n == 0:
        return np.zeros(0, dtype=dtype)
    nbytes = n * np.dtype(dtype).itemsize
    view = (C.c_char * nbytes).from_address(C.addressof(ptr.contents))
    return np.frombuffer(view, dtype=dtype).copy()


class Batch:
    """numpy copy of a freesasa_ingest_batch (field meanings: include/freesasa_ingest.h)."""

    def __init__(self, cb):
        na, nr, ns = cb.n_atoms, cb.n_residues, cb.n_structs
        self.n_structs, self.n_atoms, self.n_residues = ns, na, nr
        self.xyz = _arr(cb.xyz, 3 * na, np.float64).reshape(-1, 3)
        self.radii = _arr(cb.radii, na, np.float64)
        self.atom_class = _arr(cb.atom_class, na, np.uint8)
        self.atom_backbone = _arr(cb.atom_backbone, na, np.uint8)
        self.res_ref = _arr(cb.res_ref, nr, np.int16)
        self.atom_name_raw = np.frombuffer(C.string_at(cb.atom_name, 4 * na) if na else b"", dtype="S4").copy()
        self.atom_symbol_raw = np.frombuffer(C.string_at(cb.atom_symbol, 2 * na) if na else b"", dtype="S2").copy()
        self.offsets = _arr(cb.offsets, ns + 1, np.int64)
        self.res_first = _arr(cb.res_first, nr + 1, np.int64)
        self.res_offsets = _arr(cb.res_offsets, ns + 1, np.int64)
        self.status = _arr(cb.status, ns, np.int32)
        # residue labels stay fixed-width byte arrays until somebody asks for strings
        self.res_name_raw = np.frombuffer(C.string_at(cb.res_name, 4 * nr) if nr else b"", dtype="S4").copy()
        self.res_number_raw = np.frombuffer(C.string_at(cb.res_number, 6 * nr) if nr else b"", dtype="S6").copy()
        self.res_chain_raw = np.frombuffer(C.string_at(cb.res_chain, 4 * nr) if nr else b"", dtype="S4").copy()

    @property
    def res_name(self):
        return [v.decode() for v in self.res_name_raw.tolist()]

    @property
    def res_number(self):
        return [v.decode() for v in self.res_number_raw.tolist()]

    @property
    def res_chain(self):
        return [v.decode() for v in self.res_chain_raw.tolist()]

    def _as_c(self):
        """A freesasa_ingest_batch view of the numpy arrays (no copies; valid while self lives)."""
        cb = _CBatch()
        cb.n_structs, cb.n_atoms, cb.n_residues = self.n_structs, self.n_atoms, self.n_residues
        ptr = lambda a, t: C.cast(a.ctypes.data, C.POINTER(t))
        cb.offsets, cb.res_first, cb.res_offsets = ptr(self.offsets, C.c_int64), ptr(self.res_first, C.c_int64), ptr(self.res_offsets, C.c_int64)
        cb.atom_name, cb.atom_symbol = ptr(self.atom_name_raw, C.c_char), ptr(self.atom_symbol_raw, C.c_char)
        cb.res_name, cb.res_number, cb.res_chain = ptr(self.res_name_raw, C.c_char), ptr(self.res_number_raw, C.c_char), ptr(self.res_chain_raw, C.c_char)
        self._xyz_flat = np.ascontiguousarray(self.xyz, dtype=np.float64).reshape(-1)
        cb.xyz, cb.radii = ptr(self._xyz_flat, C.c_double), ptr(self.radii, C.c_double)
        cb.atom_class, cb.atom_backbone = ptr(self.atom_class, C.c_uint8), ptr(self.atom_backbone, C.c_uint8)
        cb.res_ref, cb.status = ptr(self.res_ref, C.c_int16), ptr(self.status, C.c_int32)
        return cb

    def save(self, path):
        """freesasa_ingest_save(): the batch as a binary cache file (load_cache() reads it back)."""
        cb = self._as_c()
        rc = _proto().freesasa_ingest_save(C.byref(cb), str(path).encode())
        if rc:
            raise RuntimeError(f"freesasa_ingest_save failed with code {rc}")

    def select(self, structure, command):
        """The reference's selection language on one structure: (name, mask[n_atoms of it], warned).
        Raises ValueError on a syntax error (the reference returns FREESASA_FAIL)."""
        L = _proto()
        n = int(self.offsets[structure + 1] - self.offsets[structure])
        mask = np.zeros(n, dtype=np.uint8)
        name = C.create_string_buffer(64)
        cb = self._as_c()
        ret = L.freesasa_ingest_select(C.byref(cb), structure, command.encode(), name, mask.ctypes.data_as(C.POINTER(C.c_ubyte)))
        if ret == -1:
            raise ValueError(f"cannot parse selection {command!r}")
        return name.value.decode(), mask, ret == -2

    def chain_groups(self, spec=None, long=False, separate_chains=False):
        """freesasa_ingest_chain_groups(): (group[n_atoms] int32, n_groups[n_structs], status[n_structs]) for
        freesasa_amd.calc_groups / GpuContext.groups.  spec: the reference's --chain-groups ("AB+C"; long=True: its
        --chain-groups-long, "A/B+C"), or separate_chains=True for one group per chain.  A structure without a
        requested chain gets status EGROUP and ids -1.  Raises ValueError on a bad spec or overlapping groups."""
        L = _proto()
        group = np.empty(self.n_atoms, dtype=np.int32)
        n_groups = np.empty(self.n_structs, dtype=np.int32)
        status = np.empty(self.n_structs, dtype=np.int32)
        err = C.create_string_buffer(256)
        flags = (GROUPS_LONG if long else 0) | (SEPARATE_CHAINS if separate_chains else 0)
        cb = self._as_c()
        i32 = C.POINTER(C.c_int32)
        ret = L.freesasa_ingest_chain_groups(C.byref(cb), spec.encode() if spec is not None else None, flags,
                                             group.ctypes.data_as(i32), n_groups.ctypes.data_as(i32),
                                             status.ctypes.data_as(i32), err, 256)
        if ret:
            raise ValueError(f"chain groups {spec!r}: {err.value.decode()}")
        return group, n_groups, status

    def residue_sums(self, per_atom):
        """Host-side segmented sum over the residues (the device-side one is GpuContext.segment_sums)."""
        per_atom = np.asarray(per_atom, dtype=np.float64)
        if self.n_residues == 0:
            return np.zeros(0)
        return np.add.reduceat(np.append(per_atom, 0.0), self.res_first[:-1])


def _proto():
    L = lib()
    if not getattr(L, "_ingest_ready", False):
        L.freesasa_ingest_pdb_files.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.POINTER(_CBatch)]
        L.freesasa_ingest_pdb_texts.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_int,
                                                C.POINTER(_CBatch)]
        L.freesasa_ingest_free.argtypes = [C.POINTER(_CBatch)]
        L.freesasa_ingest_free.restype = None
        L.freesasa_ingest_protor_radius.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_int)]
        L.freesasa_ingest_protor_radius.restype = C.c_double
        L.freesasa_ingest_guess_radius.argtypes = [C.c_char_p]
        L.freesasa_ingest_guess_radius.restype = C.c_double
        L.freesasa_ingest_residue_reference_table.argtypes = [C.POINTER(C.c_double)]
        L.freesasa_ingest_is_backbone.argtypes = [C.c_char_p]
        L.freesasa_ingest_chain_groups.argtypes = [C.POINTER(_CBatch), C.c_char_p, C.c_int, C.POINTER(C.c_int32),
                                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_char_p, C.c_int]
        L.freesasa_ingest_select.argtypes = [C.POINTER(_CBatch), C.c_int, C.c_char_p, C.c_char_p, C.POINTER(C.c_ubyte)]
        L.freesasa_ingest_save.argtypes = [C.POINTER(_CBatch), C.c_char_p]
        L.freesasa_ingest_load.argtypes = [C.c_char_p, C.POINTER(_CBatch)]
        L.freesasa_ingest_load_mt.argtypes = [C.c_char_p, C.c_int, C.POINTER(_CBatch)]
        L.freesasa_ingest_usable_cpus.restype = C.c_int
        L.freesasa_ingest_trim.argtypes = [C.c_size_t]
        L.freesasa_ingest_trim.restype = C.c_size_t
        L.freesasa_ingest_cache_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.freesasa_ingest_cache_close.argtypes = [C.c_void_p]
        L.freesasa_ingest_cache_n_structs.argtypes = [C.c_void_p]; L.freesasa_ingest_cache_n_structs.restype = C.c_int32
        L.freesasa_ingest_cache_n_atoms.argtypes = [C.c_void_p]; L.freesasa_ingest_cache_n_atoms.restype = C.c_int64
        L.freesasa_ingest_cache_offsets.argtypes = [C.c_void_p]; L.freesasa_ingest_cache_offsets.restype = C.POINTER(C.c_int64)
        L.freesasa_ingest_cache_status.argtypes = [C.c_void_p]; L.freesasa_ingest_cache_status.restype = C.POINTER(C.c_int32)
        L.freesasa_ingest_cache_read_atoms.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_ubyte)]
        L.freesasa_ingest_pdb_files_ex.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(_CBatch)]
        L.freesasa_ingest_pdb_texts_ex.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_int,
                                                   C.c_void_p, C.POINTER(_CBatch)]
        L.freesasa_ingest_classifier_from_file.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
        L.freesasa_ingest_classifier_from_file.restype = C.c_void_p
        L.freesasa_ingest_classifier_from_text.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_int]
        L.freesasa_ingest_classifier_from_text.restype = C.c_void_p
        L.freesasa_ingest_classifier_free.argtypes = [C.c_void_p]
        L.freesasa_ingest_classifier_free.restype = None
        L.freesasa_ingest_classifier_name.argtypes = [C.c_void_p]
        L.freesasa_ingest_classifier_name.restype = C.c_char_p
        L.freesasa_ingest_classifier_radius.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int)]
        L.freesasa_ingest_classifier_radius.restype = C.c_double
        L.freesasa_ingest_classifier_digest.argtypes = [C.c_void_p]
        L.freesasa_ingest_classifier_digest.restype = C.c_uint64
        L._ingest_ready = True
    return L


def _selection_proto():
    """the freesasa_ingest_selection_* entries (bound on first use: a library built before them still loads)"""
    L = _proto()
    if not getattr(L, "_selection_ready", False):
        L.freesasa_ingest_selection_compile.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_int]
        L.freesasa_ingest_selection_compile.restype = C.c_void_p
        L.freesasa_ingest_selection_count.argtypes = [C.c_void_p]
        L.freesasa_ingest_selection_name.argtypes = [C.c_void_p, C.c_int]
        L.freesasa_ingest_selection_name.restype = C.c_char_p
        L.freesasa_ingest_selection_free.argtypes = [C.c_void_p]
        L.freesasa_ingest_selection_free.restype = None
        L.freesasa_ingest_selection_program.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.freesasa_ingest_selection_program.restype = C.c_void_p
        L._selection_ready = True
    return L


def _finish(L, rc, cb):
    if rc:
        raise RuntimeError(f"freesasa_ingest failed with code {rc}")
    try:
        return Batch(cb)
    finally:
        L.freesasa_ingest_free(C.byref(cb))


class Classifier:
    """A user classifier (freesasa_ingest_classifier_*): radii and classes from a configuration file in the reference's
    format (its -c option), given as a path or as text.  Raises ValueError with the reason for a file the reference would
    reject.  .name ("no-name-given" without a name: entry), .digest (of the resolved table), .radius(res, atom) ->
    (radius, class), radius -1.0 and class UNKNOWN for an atom it does not know.  Batches loaded with one have
    res_ref = -1 throughout: a configuration file carries no reference areas."""

    def __init__(self, path=None, text=None):
        if (path is None) == (text is None):
            raise ValueError("Classifier takes exactly one of path= and text=")
        L = _proto()
        err = C.create_string_buffer(512)
        if path is not None:
            h = L.freesasa_ingest_classifier_from_file(str(path).encode(), err, len(err))
        else:
            raw = text.encode() if isinstance(text, str) else bytes(text)
            h = L.freesasa_ingest_classifier_from_text(raw, len(raw), err, len(err))
        if not h:
            raise ValueError(err.value.decode(errors="replace") or "classifier rejected")
        self._h = C.c_void_p(h)
        self.name = L.freesasa_ingest_classifier_name(self._h).decode(errors="replace")
        self.digest = int(L.freesasa_ingest_classifier_digest(self._h))

    def radius(self, res_name, atom_name):
        cls = C.c_int()
        r = _proto().freesasa_ingest_classifier_radius(self._h, _b(res_name), _b(atom_name), C.byref(cls))
        return r, cls.value

    @property
    def handle(self):
        """the freesasa_ingest_classifier * (valid while this object lives)"""
        return self._h

    def __del__(self):
        try:
            if self._h:
                _proto().freesasa_ingest_classifier_free(self._h)
                self._h = None
        except Exception:
            pass


class Selection:
    """A compiled set of 1 .. 64 selections (freesasa_ingest_selection_*): the commands of the reference's --select
    ("name, resn ala+arg and not chain B") as one program that kernels run per atom (freesasa_amd.select_batch,
    freesasa_amd.sweep_files_select).  .names (cut to 50 characters), .warned (per command: parts of it are ignored, as
    Batch.select reports).  Raises ValueError naming the command that does not parse, or the limit a set exceeds (64
    selections, 4096 program words, 64 levels of nesting); MemoryError when the library is out of memory."""

    def __init__(self, commands):
        if isinstance(commands, (str, bytes)):
            commands = [commands]
        self.commands = [c.decode() if isinstance(c, bytes) else str(c) for c in commands]
        L = _selection_proto()
        n = len(self.commands)
        arr = (C.c_char_p * max(n, 1))(*[c.encode() for c in self.commands])
        rc = (C.c_int * max(n, 1))()
        err = C.create_string_buffer(512)
        self._h = None
        h = L.freesasa_ingest_selection_compile(arr, n, rc, err, len(err))
        if not h:
            msg = err.value.decode(errors="replace") or "selection set rejected"
            if msg.startswith("out of memory"):
                raise MemoryError(msg)
            raise ValueError(msg)
        self._h = C.c_void_p(h)
        self.names = [L.freesasa_ingest_selection_name(self._h, k).decode(errors="replace") for k in range(n)]
        self.warned = [rc[k] == -2 for k in range(n)]

    def __len__(self):
        return len(self.names)

    @property
    def handle(self):
        """the freesasa_ingest_selection * (valid until close())"""
        if not self._h:
            raise ValueError("the selection set is closed")
        return self._h

    def close(self):
        if self._h:
            _selection_proto().freesasa_ingest_selection_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _b(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def _handle(classifier):
    """None -> NULL; a Classifier -> its handle"""
    if classifier is None:
        return None
    if not isinstance(classifier, Classifier):
        raise TypeError("classifier= takes an ingest.Classifier")
    return classifier.handle


def load_pdb_files(paths, options=0, n_threads=0, classifier=None):
    """Read PDB files into one Batch; per-file failures are in batch.status (empty structures).  classifier: an
    ingest.Classifier in place of ProtOr (res_ref is then -1 throughout)."""
    L = _proto()
    arr = (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])
    cb = _CBatch()
    if classifier is None:
        return _finish(L, L.freesasa_ingest_pdb_files(arr, len(paths), options, n_threads, C.byref(cb)), cb)
    return _finish(L, L.freesasa_ingest_pdb_files_ex(arr, len(paths), options, n_threads, _handle(classifier), C.byref(cb)), cb)


def load_cache(path, n_threads=0):
    """freesasa_ingest_load_mt(): a Batch from the binary cache file Batch.save() wrote, its 1 MiB pieces read and
    verified by n_threads readers (<= 0: the usable CPUs, at most 8).  Raises RuntimeError with the library's code
    (EIO: cannot open; EFORMAT: not a cache file, truncated, checksum or offsets wrong)."""
    L = _proto()
    cb = _CBatch()
    return _finish(L, L.freesasa_ingest_load_mt(str(path).encode(), int(n_threads), C.byref(cb)), cb)


def trim(keep_bytes=0):
    """freesasa_ingest_trim(): give the loader's kept blocks (freed batches, kept for the next ones: at most 1 GiB) back
    to the allocator until at most keep_bytes remain; returns the bytes released."""
    return int(_proto().freesasa_ingest_trim(int(keep_bytes)))


def usable_cpus():
    """freesasa_ingest_usable_cpus(): the affinity mask capped by the cgroup's CPU quota."""
    return int(_proto().freesasa_ingest_usable_cpus())


class Cache:
    """A cache file read partially (freesasa_ingest_cache_*): offsets and status of every structure, and
    read_atoms(a0, a1) -> (xyz, radii, atom_class) of a run of atoms, verified piece by piece."""

    def __init__(self, path):
        L = _proto()
        self._h = C.c_void_p()
        rc = L.freesasa_ingest_cache_open(str(path).encode(), C.byref(self._h))
        if rc:
            raise RuntimeError(f"freesasa_ingest_cache_open failed with code {rc}")
        self.n_structs = int(L.freesasa_ingest_cache_n_structs(self._h))
        self.n_atoms = int(L.freesasa_ingest_cache_n_atoms(self._h))
        self.offsets = np.ctypeslib.as_array(L.freesasa_ingest_cache_offsets(self._h), (self.n_structs + 1,)).copy()
        self.status = (np.ctypeslib.as_array(L.freesasa_ingest_cache_status(self._h), (self.n_structs,)).copy()
                       if self.n_structs else np.zeros(0, np.int32))

    def read_atoms(self, a0, a1):
        n = int(a1) - int(a0)
        xyz, r, cls = np.empty((max(n, 0), 3)), np.empty(max(n, 0)), np.empty(max(n, 0), np.uint8)
        rc = _proto().freesasa_ingest_cache_read_atoms(self._h, int(a0), int(a1), xyz.ctypes.data_as(C.POINTER(C.c_double)),
                                                       r.ctypes.data_as(C.POINTER(C.c_double)), cls.ctypes.data_as(C.POINTER(C.c_ubyte)))
        if rc:
            raise RuntimeError(f"freesasa_ingest_cache_read_atoms failed with code {rc}")
        return xyz, r, cls

    def close(self):
        if self._h:
            _proto().freesasa_ingest_cache_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_pdb_texts(texts, options=0, n_threads=0, classifier=None):
    """Same for PDB texts in memory (bytes or str)."""
    L = _proto()
    raw = [t.encode() if isinstance(t, str) else bytes(t) for t in texts]
    arr = (C.c_char_p * len(raw))(*raw)
    lens = (C.c_size_t * len(raw))(*[len(t) for t in raw])
    cb = _CBatch()
    if classifier is None:
        return _finish(L, L.freesasa_ingest_pdb_texts(arr, lens, len(raw), options, n_threads, C.byref(cb)), cb)
    return _finish(L, L.freesasa_ingest_pdb_texts_ex(arr, lens, len(raw), options, n_threads, _handle(classifier), C.byref(cb)), cb)


def residue_reference_table():
    """[rows, 5] reference areas (total, main chain, side chain, polar, apolar) that Batch.res_ref indexes."""
    L = _proto()
    n = L.freesasa_ingest_residue_reference_table(None)
    t = np.empty(5 * n)
    L.freesasa_ingest_residue_reference_table(t.ctypes.data_as(C.POINTER(C.c_double)))
    return t.reshape(n, 5)


load_files, load_texts = load_pdb_files, load_pdb_texts      # the format is recognised per input (PDB or mmCIF)


def protor_radius(res_name, atom_name):
    """(radius, class) of the ProtOr classifier; radius -1.0 and class UNKNOWN if the atom is not known."""
    cls = C.c_int()
    r = _proto().freesasa_ingest_protor_radius(res_name.encode(), atom_name.encode(), C.byref(cls))
    return r, cls.value


def guess_radius(symbol):
    return _proto().freesasa_ingest_guess_radius(symbol.encode())

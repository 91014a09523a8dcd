/* gpu_parse.h — what gpu_parse.hip (the device-side PDB / mmCIF parser) shares with the sweep driver. */
#ifndef FREESASA_AMD_GPU_PARSE_H
#define FREESASA_AMD_GPU_PARSE_H

#include <stddef.h>

struct freesasa_gpu_ctx;
struct freesasa_ingest_classifier;

/* rows of a user classifier the device parser takes (a larger table: the batch's files go to the host parser) */
#define PARSE_MAX_CLASSIFIER_ROWS 16384

enum { PARSE_PDB = 0, PARSE_CIF = 1, PARSE_HOST = 2 };

/* one file of a batch's text */
struct ParseFile {
    unsigned beg;          /* its first byte in the batch's text (files[F].beg = the text's length) */
    unsigned row0;         /* mmCIF: first byte (in the batch's text) of the first row of its _atom_site loop */
    short kind;            /* PARSE_PDB / PARSE_CIF / PARSE_HOST (the host parser reads it: nothing of it is looked at) */
    short ncol;            /* mmCIF: columns of the loop */
    signed char slot[12];  /* mmCIF: column of group_PDB, auth_asym_id, auth_seq_id, pdbx_PDB_ins_code, auth_comp_id, auth_atom_id,
                              label_alt_id, type_symbol, Cartn_x, Cartn_y, Cartn_z, pdbx_PDB_model_num (ingest.c cif_cols) */
    unsigned char no_final_nl; /* PDB: the file's last line had no newline (one was added behind it) */
    unsigned char pad[3];
};

/* The parser's device buffers, c->parse[] (engine_internal.h): one name per slot.  [F]: per file of the batch, [L]: per line,
   [A]: per kept atom, [R]: per residue. */
enum ParseBuf {
    PBUF_TEXT,        /* unsigned char: the batch's text, padded to 16 bytes */
    PBUF_FILES,       /* ParseFile [F + 1] */
    PBUF_BLK_CNT,     /* unsigned [text blocks + 2]: newlines per block, scanned; the last word: lines */
    PBUF_FILE_WORDS,  /* int: atoms [F] | status [F] | refused [F] */
    PBUF_FILE_OFF,    /* long long [F + 1]: a file's first kept atom */
    PBUF_LSTART,      /* unsigned [L + 2]: a line's first byte */
    PBUF_LFLAG,       /* unsigned [L] */
    PBUF_LMODEL,      /* int [L] */
    PBUF_LPOS,        /* int [L]: a kept line's place among its file's atoms */
    PBUF_LXYZR,       /* double: x [L] | y [L] | z [L] | radius [L] */
    PBUF_LCLS,        /* unsigned char [L]: class */
    PBUF_CLASSIFIER,  /* a user classifier's table: keys (uint64) | radii (double) | classes (unsigned char) */
    PBUF_AKEY,        /* uint4 [A]: residue key of every kept atom */
    PBUF_RES_BLK_CNT, /* unsigned [atom blocks + 2]: residue starts per block, scanned; the last word: residues */
    PBUF_FILE_RES0,   /* int [F]: first residue of a file that kept atoms, others -1 */
    PBUF_BACKBONE,    /* unsigned char [A + extra atoms]: backbone flags */
    PBUF_RES_FIRST,   /* int64 [R + extra residues + 1]: first atom, batch-wide */
    PBUF_RES_REF,     /* int16 [R + extra residues]: reference row (-1 throughout with a user classifier) */
    PBUF_RES_LABELS,  /* names, 4 bytes [R] | chains, 4 bytes [R] | numbers, 6 bytes [R] */
    PBUF_RES_AREAS,   /* double: abs [6 R] | rel [5 R], R with the host parser's residues (owned by the sweep, gpu_sweep.hip) */
    PBUF_ATOM_KEYS,   /* uint64 [A + extra atoms]: name (4 bytes) | symbol (2 bytes) | 0 0 of every atom, ONLY for a sweep with selections */
    PBUF_SEL_LABELS,  /* the HOST parser's residues of a selection sweep (or a loaded batch's): names, 4 bytes | chains, 4 bytes | numbers, 6 bytes */
    PBUF_SEL_PROG,    /* freesasa_sel_word: the selection set's program */
    PBUF_SEL_BITS,    /* uint64 [atoms]: bit k = selection k holds the atom */
    PBUF_SEL_OUT,     /* double [structures * selections] areas | long long [structures * selections] selected atoms */
    PBUF_COUNT
};

/* Phase 1: text -> per-file atoms / status / refused (host arrays [F]) and the total of kept atoms; cls: a user classifier
 * (NULL: ProtOr), its table uploaded with the batch.  Phase 2: the kept atoms
 * into c->h_xyz / c->h_radii / c->h_counts (classes), which are sized for total + extra_atoms first (the caller appends what
 * the host parser read of the refused files behind them).  0 / -1 (message in the context).
 * _none instead of _begin: this batch has no device-parsed part (contexts are pooled: without it _finish and the residue
 * calls would see the counts of the context's previous batch); they then only size the buffers for the extra atoms / residues. */
int parse_batch_dev_begin(freesasa_gpu_ctx *c, unsigned char *h_text, size_t T, const ParseFile *files, int F, int options,
                          const struct freesasa_ingest_classifier *cls, int *atoms_out, int *status_out, int *host_out, long long *total_atoms_out);
void parse_batch_dev_none(freesasa_gpu_ctx *c);
int parse_batch_dev_finish(freesasa_gpu_ctx *c, long long extra_atoms);

/* Residues of the atoms the device kept (freesasa_gpu_sweep_files_residues), behind parse_batch_dev_finish on the same stream,
 * by the host loader's rules (ingest.c parse_pdb / cif_visit_atom): nothing here synchronises.
 * _count: key and backbone flag of every kept atom in atom order (PBUF_BACKBONE, sized for the atoms + extra_atoms), the number
 *   of residue starts; the count is on its way into a page-locked word and is read with _found once the stream has been waited
 *   for (run_batch does).
 * _build: PBUF_RES_FIRST and PBUF_RES_REF (sized for n_res + extra_res so that the caller can append the host parser's),
 *   PBUF_RES_LABELS and PBUF_FILE_RES0. */
int parse_batch_dev_residues_count(freesasa_gpu_ctx *c, long long extra_atoms);
int parse_batch_dev_residues_found(freesasa_gpu_ctx *c);
int parse_batch_dev_residues_build(freesasa_gpu_ctx *c, int n_res, long long extra_res, int custom);

/* Atom keys of the atoms the device kept (freesasa_gpu_sweep_files_select), behind parse_batch_dev_finish on the same stream:
 * name and element symbol of every kept atom at its place in PBUF_ATOM_KEYS (sized for the atoms + extra_atoms), as the host
 * loader stores them in atom_name / atom_symbol (ingest.c parse_pdb / cif_visit_atom).  Nothing here synchronises. */
int parse_batch_dev_atom_keys(freesasa_gpu_ctx *c, long long extra_atoms);

#endif

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

/* Phase 1: text -> per-file atoms / status / refused (host arrays [F]) and the total of kept atoms; cls: a user classifier
 * (NULL: ProtOr), its table uploaded with the batch.  Phase 2: the kept atoms
 * into c->h_xyz / c->h_radii / c->h_counts (classes), which are sized for total + extra_atoms first (the caller appends what
 * the host parser read of the refused files behind them).  0 / -1 (message in the context). */
int parse_batch_dev_begin(freesasa_gpu_ctx *c, unsigned char *h_text, size_t T, const ParseFile *files, int F, int options,
                          const struct freesasa_ingest_classifier *cls, int *atoms_out, int *status_out, int *host_out, long long *total_atoms_out);
int parse_batch_dev_finish(freesasa_gpu_ctx *c, long long extra_atoms);

/* Residues of the atoms the device kept (freesasa_gpu_sweep_files_residues), behind parse_batch_dev_finish on the same stream,
 * by the host loader's rules (ingest.c parse_pdb / cif_visit_atom): nothing here synchronises.
 * _count: key and backbone flag of every kept atom in atom order (flags into c->parse[15], sized for the atoms + extra_atoms),
 *   the number of residue starts; the count is on its way into a page-locked word and is read with _found once the stream
 *   has been waited for (run_batch does).
 * _build: first atom (c->parse[16], int64 [n_res + 1], batch-wide; sized for n_res + extra_res + 1 so that the caller can
 *   append the host parser's), reference row (c->parse[17], int16; -1 throughout when custom), labels (c->parse[18]: n_res
 *   names of 4 bytes | n_res chains of 4 | n_res numbers of 6) and, per file that kept atoms, its first residue
 *   (c->parse[14], int32 [F], others -1). */
int parse_batch_dev_residues_count(freesasa_gpu_ctx *c, long long extra_atoms);
int parse_batch_dev_residues_found(freesasa_gpu_ctx *c);
int parse_batch_dev_residues_build(freesasa_gpu_ctx *c, int n_res, long long extra_res, int custom);

#endif

/* classifier.h — what the loader (ingest.c) and the device parser (gpu_parse.hip) need of a user classifier
 * (classifier.c; the public entries are in include/freesasa_ingest.h). */
#ifndef FREESASA_AMD_CLASSIFIER_H
#define FREESASA_AMD_CLASSIFIER_H

#include <stdint.h>

#include "../../include/freesasa_ingest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The lookup on tokens that are already trimmed (rl, al: their lengths): (residue, atom), then (ANY, atom).
 * Radius or -1.0; *cls the row's class or FREESASA_INGEST_UNKNOWN. */
double ingest_classifier_lookup__(const freesasa_ingest_classifier *c, const char *rt, int rl, const char *at, int al, int *cls);

/* The resolved table: rows sorted by their 7-byte key (the packing of protor_table.h: residue padded to 3 characters, atom
 * padded to 4, big-endian in the low 56 bits); *has_any: 1 if an ANY row exists.  Returns the number of rows. */
int ingest_classifier_table__(const freesasa_ingest_classifier *c, const uint64_t **keys, const double **radii,
                              const uint8_t **classes, int *has_any);

#ifdef __cplusplus
}
#endif
#endif

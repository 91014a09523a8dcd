/* classifier.c — user classifiers for the batch paths: the reference's configuration format (share/<name>.config;
 * ref: src/classifier.c:703-850, freesasa_classifier_from_file) read into one immutable, resolved table.
 * Contract: include/freesasa_ingest.h.  Host code only (gcc).
 *
 * The reader restates what the reference accepts, down to its quirks, so that a file means here what it means to the
 * reference's -c option:
 *   - a file is read in fgets chunks of at most 256 characters; a chunk of 256 that does not end a line fails the file
 *   - "types:", "atoms:" and "name:" are found as substrings of lines (the part before a '#'; a line starting with '#'
 *     has none); a section runs from where its keyword is to where the next keyword found begins
 *   - section lines lose their comment and their leading / trailing blanks; what is then shorter than two characters is
 *     an empty line
 *   - "TYPE RADIUS CLASS" and "RES ATOM TYPE" triplets (sscanf "%s %lf %s" / "%s %s %s"); residue names of at most 3
 *     characters, atom names of at most 4; the class is "apolar..." or "polar..." (prefix, case-sensitive)
 *   - a second definition of a type, or of a (residue, atom) pair, is ignored - but when it is the LAST line read of its
 *     section the reference's reader reports the warning as its section's result and rejects the whole file
 *   - an unknown type, a malformed line, a missing types: or atoms: section: the file is rejected
 *   - the name is the token behind "name:" on its line ("no-name-given" without one)
 * Lookup (ref: find_atom, src/classifier.c:739-779): (residue, atom) with both trimmed to their first token, else (ANY, atom). */
#ifndef _GNU_SOURCE
#define _GNU_SOURCE /* qsort_r */
#endif
#include "classifier.h"

#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hostfault.h"

#define MAX_LINE 256 /* the reference's MAX_LINE_LEN */
#define NO_NAME "no-name-given"

struct freesasa_ingest_classifier {
    char *name;
    int n;           /* rows */
    uint64_t *key;   /* [n] sorted */
    double *radius;  /* [n] */
    uint8_t *cls;    /* [n] */
    int has_any;
    int hash_bits;
    int32_t *hash;   /* [1 << hash_bits] row or -1 */
    uint64_t digest;
};

static inline int is_sp(char c) { return c == ' ' || (unsigned)((unsigned char)c - 9u) < 5u; }

static void set_msg(char *err, int err_len, const char *fmt, const char *arg)
{
    if (err && err_len > 0) snprintf(err, (size_t)err_len, fmt, arg ? arg : "");
}

static uint64_t pack_key(const char *res, int rl, const char *atom, int al)
{
    unsigned char b[7] = {' ', ' ', ' ', ' ', ' ', ' ', ' '};
    for (int i = 0; i < rl; ++i) b[i] = (unsigned char)res[i];
    for (int i = 0; i < al; ++i) b[3 + i] = (unsigned char)atom[i];
    uint64_t k = 0;
    for (int i = 0; i < 7; ++i) k = (k << 8) | b[i];
    return k;
}

static unsigned slot_of(uint64_t k, int bits) { return (unsigned)((k * 0x9E3779B97F4A7C15ULL) >> (64 - bits)); }

/* ------------------------------------------------------------------ the text as the reference's FILE sees it */

typedef struct { const char *p; size_t len; } text_in;

/* fgets(buf, MAX_LINE + 1) at byte `pos`: returns the position behind the chunk, or (size_t)-1 at the end of the text */
static size_t chunk_at(const text_in *t, size_t pos, char buf[MAX_LINE + 1])
{
    if (pos >= t->len) { buf[0] = '\0'; return (size_t)-1; }
    size_t n = 0;
    while (n < MAX_LINE && pos + n < t->len) {
        const char ch = t->p[pos + n];
        buf[n++] = ch;
        if (ch == '\n') break;
    }
    buf[n] = '\0';
    return pos + n;
}

/* offset of `kw` in the part of the line before a '#' (none if the line starts with '#'), -1 if absent */
static long find_keyword(const char *line, const char *kw)
{
    char buf[MAX_LINE + 1];
    if (!line[0]) return -1;
    snprintf(buf, sizeof buf, "%s", line);
    char *hash = strchr(buf, '#');
    if (hash == buf) return -1;
    if (hash) *hash = '\0';
    const char *at = strstr(buf, kw);
    return at ? (long)(at - buf) : -1;
}

/* the line without its comment and outer blanks, into out; returns its length (0: an empty line) */
static int clean_line(char *out, const char *in)
{
    char buf[MAX_LINE + 1];
    snprintf(buf, sizeof buf, "%s", in);
    char *hash = strchr(buf, '#');
    if (hash) *hash = '\0';
    long first = 0, last = (long)strlen(buf) - 1;
    while (buf[first] == ' ' || buf[first] == '\t') ++first;
    if (last > first)
        while (buf[last] == ' ' || buf[last] == '\t' || buf[last] == '\n') --last;
    if (first >= last) { out[0] = '\0'; return 0; }
    buf[last + 1] = '\0';
    snprintf(out, MAX_LINE + 1, "%s", buf + first);
    return (int)strlen(out);
}

typedef struct { long begin, end; } range;

/* ------------------------------------------------------------------ building */

typedef struct {
    /* types, in order */
    int nt, tcap;
    char **tname;
    double *trad;
    uint8_t *tcls;
    /* rows, in order of first definition, with a growing hash of their keys */
    int n, cap;
    uint64_t *key;
    double *rad;
    uint8_t *cls;
    int hbits;
    int32_t *hash;
} builder;

static void builder_free(builder *b)
{
    for (int i = 0; i < b->nt; ++i) free(b->tname[i]);
    free(b->tname); free(b->trad); free(b->tcls);
    free(b->key); free(b->rad); free(b->cls); free(b->hash);
    memset(b, 0, sizeof *b);
}

/* 0 added, 1 duplicate (ignored), -1 out of memory */
static int add_type(builder *b, const char *name, double r, int cls)
{
    for (int i = 0; i < b->nt; ++i)
        if (strcmp(b->tname[i], name) == 0) return 1;
    if (b->nt == b->tcap) {
        const int cap = b->tcap ? 2 * b->tcap : 16;
        char **tn = hf_realloc(b->tname, sizeof(char *) * (size_t)cap);
        if (!tn) return -1;
        b->tname = tn;
        double *tr = hf_realloc(b->trad, sizeof(double) * (size_t)cap);
        if (!tr) return -1;
        b->trad = tr;
        uint8_t *tc = hf_realloc(b->tcls, (size_t)cap);
        if (!tc) return -1;
        b->tcls = tc;
        b->tcap = cap;
    }
    const size_t len = strlen(name);
    char *s = hf_malloc(len + 1);
    if (!s) return -1;
    memcpy(s, name, len + 1);
    b->tname[b->nt] = s; b->trad[b->nt] = r; b->tcls[b->nt] = (uint8_t)cls;
    ++b->nt;
    return 0;
}

static int find_row(const builder *b, uint64_t k)
{
    if (!b->hash) return -1;
    for (unsigned h = slot_of(k, b->hbits);; h = (h + 1) & ((1u << b->hbits) - 1)) {
        const int i = b->hash[h];
        if (i < 0) return -1;
        if (b->key[i] == k) return i;
    }
}

static int rehash(builder *b, int bits)
{
    int32_t *h = hf_malloc(sizeof(int32_t) << bits);
    if (!h) return -1;
    for (int i = 0; i < (1 << bits); ++i) h[i] = -1;
    for (int i = 0; i < b->n; ++i) {
        unsigned s = slot_of(b->key[i], bits);
        while (h[s] >= 0) s = (s + 1) & ((1u << bits) - 1);
        h[s] = i;
    }
    free(b->hash);
    b->hash = h; b->hbits = bits;
    return 0;
}

/* 0 added, 1 duplicate (ignored), -1 out of memory */
static int add_row(builder *b, uint64_t k, double r, int cls)
{
    if (find_row(b, k) >= 0) return 1;
    if (b->n == b->cap) {
        const int cap = b->cap ? 2 * b->cap : 256;
        uint64_t *kk = hf_realloc(b->key, sizeof(uint64_t) * (size_t)cap);
        if (!kk) return -1;
        b->key = kk;
        double *rr = hf_realloc(b->rad, sizeof(double) * (size_t)cap);
        if (!rr) return -1;
        b->rad = rr;
        uint8_t *cc = hf_realloc(b->cls, (size_t)cap);
        if (!cc) return -1;
        b->cls = cc;
        b->cap = cap;
    }
    b->key[b->n] = k; b->rad[b->n] = r; b->cls[b->n] = (uint8_t)cls;
    ++b->n;
    if (2 * b->n > (b->hash ? 1 << b->hbits : 0)) {
        int bits = b->hash ? b->hbits + 1 : 9;
        while ((1 << bits) < 2 * b->n) ++bits;
        if (rehash(b, bits)) return -1;
    } else {
        unsigned s = slot_of(k, b->hbits);
        while (b->hash[s] >= 0) s = (s + 1) & ((1u << b->hbits) - 1);
        b->hash[s] = b->n - 1;
    }
    return 0;
}

enum { R_OK = 0, R_FAIL = -1, R_WARN = -2, R_NOMEM = -3 };

/* one line of the types: section (ref: read_types_line) */
static int types_line(builder *b, const char *line, char *err, int err_len)
{
    char t[MAX_LINE + 1], c[MAX_LINE + 1];
    double r;
    if (sscanf(line, "%s %lf %s", t, &r, c) != 3) {
        set_msg(err, err_len, "could not parse the line '%s' of the types: section (expected 'TYPE RADIUS CLASS')", line);
        return R_FAIL;
    }
    for (int i = 0; i < b->nt; ++i)
        if (strcmp(b->tname[i], t) == 0) return R_WARN; /* (before the class is looked at) */
    int cls;
    if (strncmp(c, "apolar", 6) == 0) cls = FREESASA_INGEST_APOLAR;
    else if (strncmp(c, "polar", 5) == 0) cls = FREESASA_INGEST_POLAR;
    else { set_msg(err, err_len, "unknown atom class '%s' (the classes are 'polar' and 'apolar')", c); return R_FAIL; }
    const int rc = add_type(b, t, r, cls);
    return rc < 0 ? R_NOMEM : (rc ? R_WARN : R_OK);
}

/* one line of the atoms: section (ref: read_atoms_line) */
static int atoms_line(builder *b, const char *line, char *err, int err_len)
{
    char res[MAX_LINE + 1], atom[MAX_LINE + 1], type[MAX_LINE + 1];
    if (sscanf(line, "%s %s %s", res, atom, type) != 3) {
        set_msg(err, err_len, "could not parse the line '%s' of the atoms: section (expected 'RESIDUE ATOM TYPE')", line);
        return R_FAIL;
    }
    if (strlen(res) > 3) { set_msg(err, err_len, "residue name '%s' is longer than 3 characters", res); return R_FAIL; }
    if (strlen(atom) > 4) { set_msg(err, err_len, "atom name '%s' is longer than 4 characters", atom); return R_FAIL; }
    int t = -1;
    for (int i = 0; i < b->nt && t < 0; ++i)
        if (strcmp(b->tname[i], type) == 0) t = i;
    if (t < 0) { set_msg(err, err_len, "unknown atom type '%s' in the atoms: section", type); return R_FAIL; }
    const int rc = add_row(b, pack_key(res, (int)strlen(res), atom, (int)strlen(atom)), b->trad[t], b->tcls[t]);
    return rc < 0 ? R_NOMEM : (rc ? R_WARN : R_OK);
}

/* the lines of a section behind its keyword line (ref: read_types / read_atoms): the result of the last line read */
static int read_section(const text_in *t, range r, const char *kw, int kwlen, builder *b,
                        int (*line_fn)(builder *, const char *, char *, int), char *err, int err_len)
{
    char raw[MAX_LINE + 1], line[MAX_LINE + 1];
    size_t pos = chunk_at(t, (size_t)r.begin, raw);
    if (pos == (size_t)-1) pos = t->len;
    if (clean_line(line, raw) == 0) { set_msg(err, err_len, "empty %s line", kw); return R_FAIL; }
    char first[MAX_LINE + 1];
    first[0] = '\0';
    sscanf(line, "%s", first);
    if (strncmp(first, kw, (size_t)kwlen) != 0 || (kwlen == 6 && strcmp(kw, "atoms:") == 0 && first[6] != '\0')) {
        /* (the reference asserts here: its keyword line starts with the keyword, and atoms: must stand alone) */
        set_msg(err, err_len, "malformed section line '%s'", line);
        return R_FAIL;
    }
    int ret = R_OK;
    while ((long)pos < r.end) {
        size_t nx = chunk_at(t, pos, raw);
        pos = nx == (size_t)-1 ? t->len : nx;
        if (clean_line(line, raw) == 0) continue;
        ret = line_fn(b, line, err, err_len);
        if (ret == R_FAIL || ret == R_NOMEM) break;
    }
    return ret;
}

static int cmp_row(const void *x, const void *y, void *unused);

static freesasa_ingest_classifier *build(const text_in *t, char *err, int err_len)
{
    char line[MAX_LINE + 1];
    range types = {-1, 0}, atoms = {-1, 0}, name = {-1, 0};
    range *last = NULL;
    /* where the sections are (ref: check_file) */
    size_t pos = 0;
    for (;;) {
        const size_t nx = chunk_at(t, pos, line);
        if (nx == (size_t)-1) break;
        range *rs[3] = {&types, &atoms, &name};
        const char *kws[3] = {"types:", "atoms:", "name:"};
        for (int k = 0; k < 3; ++k) {
            const long at = find_keyword(line, kws[k]);
            if (at < 0) continue;
            rs[k]->begin = (long)pos + at;
            if (last) last->end = (long)pos + at;
            last = rs[k];
        }
        pos = nx;
        if (strlen(line) == MAX_LINE && line[MAX_LINE - 1] != '\n') {
            set_msg(err, err_len, "a line of the classifier is longer than %s characters", "256");
            return NULL;
        }
    }
    if (last) last->end = (long)pos;
    if (types.begin < 0 || atoms.begin < 0) {
        set_msg(err, err_len, "the classifier lacks the section 'types:' or 'atoms:'%s", NULL);
        return NULL;
    }
    freesasa_ingest_classifier *c = hf_calloc(1, sizeof *c);
    if (!c) { set_msg(err, err_len, "out of memory%s", NULL); return NULL; }
    builder b;
    memset(&b, 0, sizeof b);
    int rc = R_OK;
    /* the name (ref: read_name): the token behind "name:" on its line */
    char tok[MAX_LINE + 1];
    const char *nm = NO_NAME;
    if (name.begin >= 0) {
        tok[0] = '\0';
        size_t nx = chunk_at(t, (size_t)name.begin, line);
        if (nx != (size_t)-1) sscanf(line, "%s", tok);
        if (strcmp(tok, "name:") != 0) { set_msg(err, err_len, "malformed name line '%s'", line); rc = R_FAIL; }
        else {
            tok[0] = '\0';
            nx = chunk_at(t, (size_t)name.begin + 5, line);
            if (nx != (size_t)-1) sscanf(line, "%s", tok);
            if (!tok[0]) { set_msg(err, err_len, "empty name for the classifier%s", NULL); rc = R_FAIL; }
            nm = tok;
        }
    }
    if (rc == R_OK) {
        c->name = hf_malloc(strlen(nm) + 1);
        if (!c->name) rc = R_NOMEM;
        else strcpy(c->name, nm);
    }
    if (rc == R_OK) rc = read_section(t, types, "types:", 6, &b, types_line, err, err_len);
    if (rc == R_OK) rc = read_section(t, atoms, "atoms:", 6, &b, atoms_line, err, err_len);
    if (rc == R_WARN) set_msg(err, err_len, "the last line of a section repeats an earlier definition (the reference rejects such a file)%s", NULL);
    if (rc == R_OK) {
        /* the resolved table: rows sorted by key, and an open-addressing hash of them */
        const int n = b.n;
        int *order = hf_malloc(sizeof(int) * (size_t)(n ? n : 1));
        c->key = hf_malloc(sizeof(uint64_t) * (size_t)(n ? n : 1));
        c->radius = hf_malloc(sizeof(double) * (size_t)(n ? n : 1));
        c->cls = hf_malloc((size_t)(n ? n : 1));
        int bits = 4;
        while ((1 << bits) < 2 * n) ++bits;
        c->hash = hf_malloc(sizeof(int32_t) << bits);
        if (!order || !c->key || !c->radius || !c->cls || !c->hash) rc = R_NOMEM;
        else {
            for (int i = 0; i < n; ++i) order[i] = i;
            qsort_r(order, (size_t)n, sizeof(int), cmp_row, b.key);
            const uint64_t any = pack_key("ANY", 3, "", 0) >> 32;
            uint64_t h = 1469598103934665603ULL; /* FNV-1a over the rows: the table's content, not the text's */
            c->n = n; c->hash_bits = bits;
            for (int i = 0; i < n; ++i) {
                c->key[i] = b.key[order[i]]; c->radius[i] = b.rad[order[i]]; c->cls[i] = b.cls[order[i]];
                if ((c->key[i] >> 32) == any) c->has_any = 1;
                unsigned char row[17];
                memcpy(row, &c->key[i], 8); memcpy(row + 8, &c->radius[i], 8); row[16] = c->cls[i];
                for (int q = 0; q < 17; ++q) h = (h ^ row[q]) * 1099511628211ULL;
            }
            c->digest = h ^ (h >> 29) ^ ((uint64_t)n << 40);
            for (int i = 0; i < (1 << bits); ++i) c->hash[i] = -1;
            for (int i = 0; i < n; ++i) {
                unsigned s = slot_of(c->key[i], bits);
                while (c->hash[s] >= 0) s = (s + 1) & ((1u << bits) - 1);
                c->hash[s] = i;
            }
        }
        free(order);
    }
    builder_free(&b);
    if (rc != R_OK) {
        if (rc == R_NOMEM) set_msg(err, err_len, "out of memory%s", NULL);
        freesasa_ingest_classifier_free(c);
        return NULL;
    }
    return c;
}

static int cmp_row(const void *x, const void *y, void *keys)
{
    const uint64_t a = ((const uint64_t *)keys)[*(const int *)x], b = ((const uint64_t *)keys)[*(const int *)y];
    return a < b ? -1 : (a > b);
}

/* ------------------------------------------------------------------ entry points */

freesasa_ingest_classifier *freesasa_ingest_classifier_from_text(const char *text, size_t len, char *err, int err_len)
{
    if (err && err_len > 0) err[0] = '\0';
    if (!text) { set_msg(err, err_len, "null text%s", NULL); return NULL; }
    const text_in t = {text, len};
    return build(&t, err, err_len);
}

freesasa_ingest_classifier *freesasa_ingest_classifier_from_file(const char *path, char *err, int err_len)
{
    if (err && err_len > 0) err[0] = '\0';
    if (!path) { set_msg(err, err_len, "null path%s", NULL); return NULL; }
    FILE *fp = fopen(path, "rb");
    if (!fp) { if (err && err_len > 0) snprintf(err, (size_t)err_len, "cannot open '%s': %s", path, strerror(errno)); return NULL; }
    size_t cap = 1 << 14, len = 0;
    char *buf = hf_malloc(cap);
    int ok = buf != NULL;
    while (ok) {
        if (len == cap) {
            char *nb = hf_realloc(buf, 2 * cap);
            if (!nb) { ok = 0; break; }
            buf = nb; cap *= 2;
        }
        const size_t got = fread(buf + len, 1, cap - len, fp);
        len += got;
        if (got == 0) { if (ferror(fp)) ok = -1; break; }
    }
    fclose(fp);
    if (ok != 1) {
        free(buf);
        if (ok < 0 && err && err_len > 0) snprintf(err, (size_t)err_len, "cannot read '%s'", path);
        else set_msg(err, err_len, "out of memory%s", NULL);
        return NULL;
    }
    const text_in t = {buf, len};
    freesasa_ingest_classifier *c = build(&t, err, err_len);
    free(buf);
    return c;
}

void freesasa_ingest_classifier_free(freesasa_ingest_classifier *c)
{
    if (!c) return;
    free(c->name); free(c->key); free(c->radius); free(c->cls); free(c->hash);
    free(c);
}

const char *freesasa_ingest_classifier_name(const freesasa_ingest_classifier *c) { return c ? c->name : NULL; }

uint64_t freesasa_ingest_classifier_digest(const freesasa_ingest_classifier *c) { return c ? c->digest : 0; }

static inline int find(const freesasa_ingest_classifier *c, uint64_t k)
{
    for (unsigned h = slot_of(k, c->hash_bits);; h = (h + 1) & ((1u << c->hash_bits) - 1)) {
        const int i = c->hash[h];
        if (i < 0 || c->key[i] == k) return i;
    }
}

double ingest_classifier_lookup__(const freesasa_ingest_classifier *c, const char *rt, int rl, const char *at, int al, int *cls)
{
    *cls = FREESASA_INGEST_UNKNOWN;
    if (al < 1 || al > 4) return -1.0;
    int i = -1;
    if (rl >= 1 && rl <= 3) i = find(c, pack_key(rt, rl, at, al));
    if (i < 0 && c->has_any) i = find(c, pack_key("ANY", 3, at, al)); /* a residue not listed, or listed without the atom */
    if (i < 0) return -1.0;
    *cls = c->cls[i];
    return c->radius[i];
}

double freesasa_ingest_classifier_radius(const freesasa_ingest_classifier *c, const char *res_name, const char *atom_name, int *cls)
{
    int k = FREESASA_INGEST_UNKNOWN;
    double r = -1.0;
    if (c && res_name && atom_name) {
        const char *rt = res_name, *at = atom_name;
        while (*rt && is_sp(*rt)) ++rt;
        while (*at && is_sp(*at)) ++at;
        int rl = 0, al = 0;
        while (rt[rl] && !is_sp(rt[rl])) ++rl;
        while (at[al] && !is_sp(at[al])) ++al;
        r = ingest_classifier_lookup__(c, rt, rl, at, al, &k);
    }
    if (cls) *cls = k;
    return r;
}

int ingest_classifier_table__(const freesasa_ingest_classifier *c, const uint64_t **keys, const double **radii,
                              const uint8_t **classes, int *has_any)
{
    *keys = c->key; *radii = c->radius; *classes = c->cls; *has_any = c->has_any;
    return c->n;
}

/* select.c — the reference's selection language on a loaded batch.
 *
 *     "name, expr"    expr := resn LIST | resi RANGES | symbol LIST | name LIST | chain RANGES
 *                             | expr and expr | expr or expr | not expr | ( expr )
 *
 * Restates the reference's lexer (src/lexer.l: longest match, first rule wins ties, unknown
 * characters are skipped), grammar (src/parser.y: or < and < not; '+' joins list items; '-' makes
 * ranges, open on either side for residue numbers; "\-" is a minus sign) and evaluation
 * (src/selection.c:283-660: identifiers are upper-cased, names/residue names/numbers/symbols are
 * compared with the structure's trimmed fields, ranges use atoi of the residue number or the
 * chain character, invalid identifiers are ignored with a warning).  The result is a byte mask over
 * the atoms of one structure of a freesasa_ingest_batch; the area of a selection is the masked sum
 * of per-atom SASA (freesasa_gpu_class_sums_dev with the mask as class gives it on the device).
 * Host code only; freesasa_ingest_selection_compile (below) turns a set of commands into a program that kernels run.
 */
#include "freesasa_ingest.h"

#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hostfault.h"
#include "select_program.h"

/* ------------------------------------------------------------------ lexer */

enum { K_END, K_COMMA, K_DASH, K_PLUS, K_LPAR, K_RPAR, K_RESN, K_RESI, K_SYMBOL, K_NAME, K_CHAIN, K_AND, K_OR, K_NOT,
       K_MINUS, K_NUMBER, K_ID, K_SELID };
typedef struct { int type; char text[64]; } tok_t;
typedef struct { const char *s; size_t pos, len; } lex_t;

static size_t match_ci(const char *p, size_t left, const char *word)
{
    const size_t n = strlen(word);
    if (left < n) return 0;
    for (size_t i = 0; i < n; ++i)
        if (tolower((unsigned char)p[i]) != word[i]) return 0;
    return n;
}
static int is_idc(int c) { return isalnum(c) || c == '_'; }

/* the next token by flex's rules: among all patterns the longest match, the earlier rule on a tie */
static tok_t next_token(lex_t *lx)
{
    tok_t t;
    t.text[0] = '\0';
    for (;;) {
        if (lx->pos >= lx->len) { t.type = K_END; return t; }
        const char *p = lx->s + lx->pos;
        const size_t left = lx->len - lx->pos;
        size_t best = 0, take = 0;
        int type = -1;
#define CAND(n_, ty_) do { const size_t n__ = (n_); if (n__ > best) { best = n__; take = n__; type = (ty_); } } while (0)
        CAND(p[0] == ',', K_COMMA);
        CAND(p[0] == '-', K_DASH);
        CAND(p[0] == '+', K_PLUS);
        CAND(p[0] == '(', K_LPAR);
        CAND(p[0] == ')', K_RPAR);
        CAND(match_ci(p, left, "resn"), K_RESN);
        CAND(match_ci(p, left, "resi"), K_RESI);
        CAND(match_ci(p, left, "symbol"), K_SYMBOL);
        CAND(match_ci(p, left, "name"), K_NAME);
        CAND(match_ci(p, left, "chain"), K_CHAIN);
        CAND(p[0] == '&' ? 1 : match_ci(p, left, "and"), K_AND);
        CAND(p[0] == '|' ? 1 : match_ci(p, left, "or"), K_OR);
        CAND(p[0] == '!' ? 1 : match_ci(p, left, "not"), K_NOT);
        CAND(left >= 2 && p[0] == '\\' && p[1] == '-' ? 2 : 0, K_MINUS);
        size_t ws = 0;
        while (ws < left && (p[ws] == ' ' || p[ws] == '\t' || p[ws] == '\n' || p[ws] == '\r')) ++ws;
        CAND(ws, -2);
        size_t nd = 0;
        while (nd < left && isdigit((unsigned char)p[nd])) ++nd;
        CAND(nd, K_NUMBER);
        size_t ni = 0;
        while (ni < left && is_idc((unsigned char)p[ni])) ++ni;
        if (ni) while (ni < left && p[ni] == '\'') ++ni;
        CAND(ni, K_ID);
        size_t nsel = 0; /* [[:alnum:]_\-\+]+ followed by ',': the comma counts for the length, not for the text */
        while (nsel < left && (is_idc((unsigned char)p[nsel]) || p[nsel] == '-' || p[nsel] == '+')) ++nsel;
        if (nsel && nsel < left && p[nsel] == ',' && nsel + 1 > best) { best = nsel + 1; take = nsel; type = K_SELID; }
#undef CAND
        if (type == -1) { lx->pos += 1; continue; } /* flex's default rule: the character is echoed and dropped */
        lx->pos += take;
        if (type == -2) continue;
        t.type = type;
        const size_t n = take < sizeof t.text - 1 ? take : sizeof t.text - 1;
        memcpy(t.text, p, n);
        t.text[n] = '\0';
        return t;
    }
}

/* ------------------------------------------------------------------ parser */

enum { E_AND, E_OR, E_NOT, E_RESN, E_RESI, E_SYMBOL, E_NAME, E_CHAIN, E_PLUS, E_RANGE, E_RANGE_OPEN_L, E_RANGE_OPEN_R,
       E_NUMBER, E_ID };
typedef struct expr { int type; struct expr *l, *r; char value[64]; } expr;

typedef struct { lex_t lx; tok_t cur; int err; } parser;

static void advance(parser *ps) { ps->cur = next_token(&ps->lx); }
static expr *node(int type, expr *l, expr *r)
{
    expr *e = hf_calloc(1, sizeof *e);
    if (e) { e->type = type; e->l = l; e->r = r; }
    return e;
}
static void free_expr(expr *e)
{
    if (!e) return;
    free_expr(e->l); free_expr(e->r); free(e);
}

/* id: NUMBER | ID | "\-" NUMBER; values are upper-cased (ref: src/selection.c:100-131) */
static expr *parse_id(parser *ps)
{
    expr *e = NULL;
    if (ps->cur.type == K_NUMBER || ps->cur.type == K_ID) {
        e = node(ps->cur.type == K_NUMBER ? E_NUMBER : E_ID, NULL, NULL);
        if (e) snprintf(e->value, sizeof e->value, "%s", ps->cur.text);
        advance(ps);
    } else if (ps->cur.type == K_MINUS) {
        advance(ps);
        if (ps->cur.type != K_NUMBER) { ps->err = 1; return NULL; }
        e = node(E_NUMBER, NULL, NULL);
        if (e) snprintf(e->value, sizeof e->value, "-%.60s", ps->cur.text);
        advance(ps);
    } else {
        ps->err = 1;
        return NULL;
    }
    if (e) for (char *c = e->value; *c; ++c) *c = (char)toupper((unsigned char)*c);
    else ps->err = 1;
    return e;
}
static int starts_id(const parser *ps) { return ps->cur.type == K_NUMBER || ps->cur.type == K_ID || ps->cur.type == K_MINUS; }

static expr *parse_list(parser *ps) /* id ('+' id)*, right-nested like the grammar */
{
    expr *left = parse_id(ps);
    if (!left) return NULL;
    if (ps->cur.type == K_PLUS) {
        advance(ps);
        expr *right = parse_list(ps);
        if (!right) { free_expr(left); return NULL; }
        return node(E_PLUS, left, right);
    }
    return left;
}

/* one item of a range list: id | id '-' id | '-' id | id '-' (the open forms only for residues) */
static expr *parse_range_item(parser *ps, int allow_open)
{
    if (ps->cur.type == K_DASH) {
        if (!allow_open) { ps->err = 1; return NULL; }
        advance(ps);
        expr *right = parse_id(ps);
        return right ? node(E_RANGE_OPEN_L, NULL, right) : NULL;
    }
    expr *left = parse_id(ps);
    if (!left) return NULL;
    if (ps->cur.type == K_DASH) {
        advance(ps);
        if (starts_id(ps)) {
            expr *right = parse_id(ps);
            if (!right) { free_expr(left); return NULL; }
            return node(E_RANGE, left, right);
        }
        if (!allow_open) { ps->err = 1; free_expr(left); return NULL; }
        return node(E_RANGE_OPEN_R, left, NULL);
    }
    return left;
}
static expr *parse_ranges(parser *ps, int allow_open) /* item ('+' item)*, left-associative */
{
    expr *left = parse_range_item(ps, allow_open);
    while (left && ps->cur.type == K_PLUS) {
        advance(ps);
        expr *right = parse_range_item(ps, allow_open);
        if (!right) { free_expr(left); return NULL; }
        left = node(E_PLUS, left, right);
    }
    /* "1-2-3", "1-2-": a second dash after a complete item is a syntax error in the grammar */
    if (left && ps->cur.type == K_DASH) { ps->err = 1; free_expr(left); return NULL; }
    return left;
}

static expr *parse_or(parser *ps);
static expr *parse_primary(parser *ps)
{
    switch (ps->cur.type) {
    case K_LPAR: {
        advance(ps);
        expr *e = parse_or(ps);
        if (!e) return NULL;
        if (ps->cur.type != K_RPAR) { ps->err = 1; free_expr(e); return NULL; }
        advance(ps);
        return e;
    }
    case K_NOT: {
        advance(ps);
        expr *e = parse_primary(ps); /* not binds tighter than and / or */
        return e ? node(E_NOT, NULL, e) : NULL;
    }
    case K_RESN: { advance(ps); expr *l = parse_list(ps); return l ? node(E_RESN, l, NULL) : NULL; }
    case K_SYMBOL: { advance(ps); expr *l = parse_list(ps); return l ? node(E_SYMBOL, l, NULL) : NULL; }
    case K_NAME: { advance(ps); expr *l = parse_list(ps); return l ? node(E_NAME, l, NULL) : NULL; }
    case K_RESI: { advance(ps); expr *l = parse_ranges(ps, 1); return l ? node(E_RESI, l, NULL) : NULL; }
    case K_CHAIN: { advance(ps); expr *l = parse_ranges(ps, 0); return l ? node(E_CHAIN, l, NULL) : NULL; }
    default:
        ps->err = 1;
        return NULL;
    }
}
static expr *parse_and(parser *ps)
{
    expr *left = parse_primary(ps);
    while (left && ps->cur.type == K_AND) {
        advance(ps);
        expr *right = parse_primary(ps);
        if (!right) { free_expr(left); return NULL; }
        left = node(E_AND, left, right);
    }
    return left;
}
static expr *parse_or(parser *ps)
{
    expr *left = parse_and(ps);
    while (left && ps->cur.type == K_OR) {
        advance(ps);
        expr *right = parse_and(ps);
        if (!right) { free_expr(left); return NULL; }
        left = node(E_OR, left, right);
    }
    return left;
}

/* ------------------------------------------------------------------ evaluation */

typedef struct {
    const freesasa_ingest_batch *b;
    int64_t a0, n;     /* atoms of the structure */
    const int64_t *res; /* residue index of every atom of the structure */
    int warn;
} ctx_t;

static void trimmed(char *dst, size_t cap, const char *src, size_t w)
{
    size_t i = 0, n = 0;
    while (i < w && src[i] && isspace((unsigned char)src[i])) ++i;
    while (i < w && src[i] && !isspace((unsigned char)src[i]) && n + 1 < cap) dst[n++] = src[i++];
    dst[n] = '\0';
}
static void atom_field(const ctx_t *c, int64_t i, int parent, char *out, size_t cap)
{
    const freesasa_ingest_batch *b = c->b;
    const int64_t a = c->a0 + i, r = c->res[i];
    switch (parent) {
    case E_NAME: trimmed(out, cap, b->atom_name + 4 * a, 4); break;
    case E_SYMBOL: trimmed(out, cap, b->atom_symbol + 2 * a, 2); break;
    case E_RESN: trimmed(out, cap, b->res_name + 4 * r, 4); break;
    default: trimmed(out, cap, b->res_number + 6 * r, 6); break; /* E_RESI */
    }
}
static int resnum(const ctx_t *c, int64_t i) /* atoi of the residue number field */
{
    char buf[8];
    memcpy(buf, c->b->res_number + 6 * c->res[i], 6);
    buf[6] = '\0';
    return atoi(buf);
}

/* ref: src/selection.c:376-452 */
static int valid_id(int parent, const expr *e)
{
    const char *v = e->value;
    const size_t n = strlen(v);
    switch (parent) {
    case E_NAME: return n <= 4;
    case E_SYMBOL: return e->type == E_ID && n <= 2;
    case E_RESN: return n <= 3;
    case E_RESI:
        if (e->type == E_NUMBER) return 1;
        if (n > 5 || n == 1) return 0;
        if (toupper((unsigned char)v[n - 1]) < 'A' || toupper((unsigned char)v[n - 1]) > 'Z') return 0;
        for (size_t i = 0; i + 1 < n; ++i)
            if (v[i] < '0' || v[i] > '9') return 0;
        return 1;
    default: return n <= 1; /* E_CHAIN */
    }
}

static void select_id(ctx_t *c, int parent, const char *id, unsigned char *mask)
{
    char f[16];
    for (int64_t i = 0; i < c->n; ++i) {
        int m;
        if (parent == E_CHAIN) m = id[0] == c->b->res_chain[4 * c->res[i]];
        else { atom_field(c, i, parent, f, sizeof f); m = strcmp(f, id) == 0; }
        if (m) mask[i] = 1;
    }
}

/* ref: src/selection.c:454-505 */
static void select_range(ctx_t *c, int type, int parent, const expr *l, const expr *r, unsigned char *mask)
{
    if (parent == E_RESI) {
        if ((l && l->type != E_NUMBER) || (r && r->type != E_NUMBER)) { c->warn = 1; return; }
    } else {
        if (l->type != r->type || (l->type == E_ID && (strlen(l->value) > 1 || strlen(r->value) > 1))) { c->warn = 1; return; }
    }
    int lower, upper;
    if (type == E_RANGE_OPEN_L) { lower = resnum(c, 0); upper = atoi(r->value); }
    else if (type == E_RANGE_OPEN_R) { lower = atoi(l->value); upper = resnum(c, c->n - 1); }
    else if (l->type == E_NUMBER) { lower = atoi(l->value); upper = atoi(r->value); }
    else { lower = (int)l->value[0]; upper = (int)r->value[0]; }
    for (int64_t i = 0; i < c->n; ++i) {
        const int j = parent == E_RESI ? resnum(c, i) : (int)c->b->res_chain[4 * c->res[i]];
        if (j >= lower && j <= upper) mask[i] = 1;
    }
}

static void select_list(ctx_t *c, int parent, const expr *e, unsigned char *mask)
{
    switch (e->type) {
    case E_PLUS: select_list(c, parent, e->l, mask); select_list(c, parent, e->r, mask); break;
    case E_RANGE: case E_RANGE_OPEN_L: case E_RANGE_OPEN_R: select_range(c, e->type, parent, e->l, e->r, mask); break;
    default: /* E_ID, E_NUMBER */
        if (valid_id(parent, e)) select_id(c, parent, e->value, mask);
        else c->warn = 1;
    }
}

static int eval(ctx_t *c, const expr *e, unsigned char *mask)
{
    memset(mask, 0, (size_t)c->n);
    switch (e->type) {
    case E_RESN: case E_RESI: case E_SYMBOL: case E_NAME: case E_CHAIN:
        select_list(c, e->type, e->l, mask);
        return 0;
    case E_NOT:
        if (eval(c, e->r, mask)) return -1;
        for (int64_t i = 0; i < c->n; ++i) mask[i] = !mask[i];
        return 0;
    default: { /* E_AND, E_OR */
        unsigned char *tmp = hf_malloc((size_t)(c->n ? c->n : 1));
        if (!tmp) return -1;
        int rc = eval(c, e->l, mask) || eval(c, e->r, tmp);
        if (!rc)
            for (int64_t i = 0; i < c->n; ++i) mask[i] = e->type == E_AND ? (mask[i] && tmp[i]) : (mask[i] || tmp[i]);
        free(tmp);
        return rc ? -1 : 0;
    }
    }
}

int freesasa_ingest_select(const freesasa_ingest_batch *b, int structure, const char *command,
                           char name_out[FREESASA_INGEST_MAX_SELECTION_NAME + 1], unsigned char *mask_out)
{
    if (!b || !command || !name_out || !mask_out || structure < 0 || structure >= b->n_structs) return FREESASA_INGEST_SELECT_FAIL;
    name_out[0] = '\0';
    parser ps;
    memset(&ps, 0, sizeof ps);
    ps.lx.s = command; ps.lx.len = strlen(command);
    advance(&ps);
    if (ps.cur.type != K_SELID) return FREESASA_INGEST_SELECT_FAIL;
    char name[64];
    snprintf(name, sizeof name, "%s", ps.cur.text);
    advance(&ps);
    if (ps.cur.type != K_COMMA) return FREESASA_INGEST_SELECT_FAIL;
    advance(&ps);
    expr *e = parse_or(&ps);
    if (!e || ps.err || ps.cur.type != K_END) { free_expr(e); return FREESASA_INGEST_SELECT_FAIL; }

    ctx_t c;
    c.b = b; c.a0 = b->offsets[structure]; c.n = b->offsets[structure + 1] - c.a0; c.warn = 0;
    if (c.n == 0) { /* an input that failed to load: nothing to select from */
        free_expr(e);
        snprintf(name_out, FREESASA_INGEST_MAX_SELECTION_NAME + 1, "%.50s", name);
        return 0;
    }
    int64_t *res = hf_malloc(sizeof(int64_t) * (size_t)c.n);
    if (!res) { free_expr(e); return FREESASA_INGEST_SELECT_FAIL; }
    for (int64_t r = b->res_offsets[structure]; r < b->res_offsets[structure + 1]; ++r)
        for (int64_t a = b->res_first[r]; a < b->res_first[r + 1]; ++a) res[a - c.a0] = r;
    c.res = res;
    const int rc = eval(&c, e, mask_out);
    free(res);
    free_expr(e);
    if (rc) return FREESASA_INGEST_SELECT_FAIL;
    snprintf(name_out, FREESASA_INGEST_MAX_SELECTION_NAME + 1, "%.50s", name);
    return c.warn ? FREESASA_INGEST_SELECT_WARN : (int)c.n;
}

/* ------------------------------------------------------------------ compiled selection sets (select_program.h)
 * The same lexer, parser and rules; the tree of every command flattened into one postfix program that a kernel runs per
 * atom (select_kernels.h).  freesasa_ingest_select above is what the program is held against. */

struct freesasa_ingest_selection {
    int n, n_words, flags, depth;
    char name[SEL_MAX_SELECTIONS][FREESASA_INGEST_MAX_SELECTION_NAME + 1];
    freesasa_sel_word words[SEL_MAX_WORDS];
};

typedef struct { freesasa_ingest_selection *s; int warn, too_long, depth; } comp_t;

static void emit(comp_t *c, uint32_t op, uint32_t a, uint32_t b)
{
    freesasa_ingest_selection *s = c->s;
    if (s->n_words >= SEL_MAX_WORDS) { c->too_long = 1; return; }
    freesasa_sel_word *w = &s->words[s->n_words++];
    w->op = op; w->a = a; w->b = b; w->c = 0;
    if (op == SEL_OP_AND || op == SEL_OP_OR || op == SEL_OP_END) --c->depth;
    else if (op != SEL_OP_NOT && ++c->depth > s->depth) s->depth = c->depth;
}

/* select_id: an id that valid_id refuses is skipped with a warning; the others compare with a trimmed field */
static void comp_id(comp_t *c, int parent, const expr *e)
{
    if (!valid_id(parent, e)) { c->warn = 1; emit(c, SEL_OP_FALSE, 0, 0); return; }
    if (parent == E_CHAIN) { emit(c, SEL_OP_CHAIN, (unsigned char)e->value[0], 0); return; }
    const size_t n = strlen(e->value);
    if (n > 6) { emit(c, SEL_OP_FALSE, 0, 0); return; } /* (a number longer than the number field: equals no field) */
    uint64_t key = 0;
    for (size_t i = 0; i < n; ++i) key |= (uint64_t)(unsigned char)e->value[i] << (8 * i);
    const uint32_t op = parent == E_NAME ? SEL_OP_NAME : parent == E_SYMBOL ? SEL_OP_SYMBOL : parent == E_RESN ? SEL_OP_RESN : SEL_OP_RESI;
    emit(c, op, (uint32_t)key, (uint32_t)(key >> 32));
}

/* select_range: its type checks, its bounds */
static void comp_range(comp_t *c, int type, int parent, const expr *l, const expr *r)
{
    int bad;
    if (parent == E_RESI) bad = (l && l->type != E_NUMBER) || (r && r->type != E_NUMBER);
    else bad = l->type != r->type || (l->type == E_ID && (strlen(l->value) > 1 || strlen(r->value) > 1));
    if (bad) { c->warn = 1; emit(c, SEL_OP_FALSE, 0, 0); return; }
    if (parent == E_RESI) {
        c->s->flags |= SEL_FLAG_RESI_RANGE;
        if (type == E_RANGE_OPEN_L) { c->s->flags |= SEL_FLAG_OPEN; emit(c, SEL_OP_RESI_OPEN_L, 0, (uint32_t)atoi(r->value)); }
        else if (type == E_RANGE_OPEN_R) { c->s->flags |= SEL_FLAG_OPEN; emit(c, SEL_OP_RESI_OPEN_R, (uint32_t)atoi(l->value), 0); }
        else emit(c, SEL_OP_RESI_RANGE, (uint32_t)atoi(l->value), (uint32_t)atoi(r->value));
    } else if (l->type == E_NUMBER) {
        emit(c, SEL_OP_CHAIN_RANGE, (uint32_t)atoi(l->value), (uint32_t)atoi(r->value)); /* ("chain 1-5": the character's code in 1..5) */
    } else {
        emit(c, SEL_OP_CHAIN_RANGE, (uint32_t)(int)l->value[0], (uint32_t)(int)r->value[0]);
    }
}

/* select_list: the items in its order, joined by or (*count: items so far) */
static void comp_list(comp_t *c, int parent, const expr *e, int *count)
{
    if (e->type == E_PLUS) { comp_list(c, parent, e->l, count); comp_list(c, parent, e->r, count); return; }
    if (e->type == E_RANGE || e->type == E_RANGE_OPEN_L || e->type == E_RANGE_OPEN_R) comp_range(c, e->type, parent, e->l, e->r);
    else comp_id(c, parent, e);
    if ((*count)++) emit(c, SEL_OP_OR, 0, 0);
}

static void comp_expr(comp_t *c, const expr *e)
{
    switch (e->type) {
    case E_RESN: case E_RESI: case E_SYMBOL: case E_NAME: case E_CHAIN: {
        int count = 0;
        comp_list(c, e->type, e->l, &count);
        break;
    }
    case E_NOT: comp_expr(c, e->r); emit(c, SEL_OP_NOT, 0, 0); break;
    default: comp_expr(c, e->l); comp_expr(c, e->r); emit(c, e->type == E_AND ? SEL_OP_AND : SEL_OP_OR, 0, 0); break;
    }
}

static freesasa_ingest_selection *sel_fail(freesasa_ingest_selection *s, char *err, int err_len, const char *fmt, const char *arg)
{
    if (err && err_len > 0) snprintf(err, (size_t)err_len, fmt, arg);
    free(s);
    return NULL;
}

freesasa_ingest_selection *freesasa_ingest_selection_compile(const char *const *commands, int n_commands, int *rc_out, char *err, int err_len)
{
    if (err && err_len > 0) err[0] = '\0';
    if (!commands || n_commands < 1) return sel_fail(NULL, err, err_len, "%s", "no selection commands given");
    for (int k = 0; rc_out && k < n_commands; ++k) rc_out[k] = 0;
    if (n_commands > SEL_MAX_SELECTIONS) return sel_fail(NULL, err, err_len, "%s", "more than 64 selections in one set");
    freesasa_ingest_selection *s = hf_calloc(1, sizeof *s);
    if (!s) return sel_fail(NULL, err, err_len, "%s", "out of memory (selection set)");
    for (int k = 0; k < n_commands; ++k) {
        const char *command = commands[k];
        parser ps; /* (the head of a command as freesasa_ingest_select reads it) */
        memset(&ps, 0, sizeof ps);
        expr *e = NULL;
        char name[64] = "";
        if (command) {
            ps.lx.s = command; ps.lx.len = strlen(command);
            advance(&ps);
            if (ps.cur.type == K_SELID) {
                snprintf(name, sizeof name, "%s", ps.cur.text);
                advance(&ps);
                if (ps.cur.type == K_COMMA) { advance(&ps); e = parse_or(&ps); }
            }
        }
        if (!e || ps.err || ps.cur.type != K_END) {
            free_expr(e);
            if (rc_out) rc_out[k] = FREESASA_INGEST_SELECT_FAIL;
            return sel_fail(s, err, err_len, "cannot parse selection '%.200s'", command ? command : "(null)");
        }
        comp_t c;
        c.s = s; c.warn = 0; c.too_long = 0; c.depth = 0;
        comp_expr(&c, e);
        emit(&c, SEL_OP_END, (uint32_t)k, 0);
        free_expr(e);
        if (c.too_long) return sel_fail(s, err, err_len, "the selection set is longer than a program of 4096 words (at '%.200s')", command);
        if (s->depth > SEL_MAX_DEPTH) return sel_fail(s, err, err_len, "selection '%.200s' is nested deeper than 64 levels", command);
        if (c.warn && rc_out) rc_out[k] = FREESASA_INGEST_SELECT_WARN;
        snprintf(s->name[k], sizeof s->name[k], "%.50s", name);
        s->n = k + 1;
    }
    return s;
}

int freesasa_ingest_selection_count(const freesasa_ingest_selection *s) { return s ? s->n : 0; }
const char *freesasa_ingest_selection_name(const freesasa_ingest_selection *s, int k) { return s && k >= 0 && k < s->n ? s->name[k] : NULL; }
void freesasa_ingest_selection_free(freesasa_ingest_selection *s) { free(s); }
const void *freesasa_ingest_selection_program(const freesasa_ingest_selection *s, int *n_words, int *flags)
{
    if (!s) return NULL;
    if (n_words) *n_words = s->n_words;
    if (flags) *flags = s->flags;
    return s->words;
}

/* ------------------------------------------------------------------ chain groups (include/freesasa_ingest.h) */

#define CG_MAX_LABELS 4096
typedef struct { char label[4]; int group; } cg_label_t;

static int cg_fail(char *err, int err_len, const char *msg)
{
    if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", msg);
    return -1;
}

/* The tokens of the reference's split() (src/main.cc:380-386: std::sregex_token_iterator with -1): text between the
 * separators, an empty one between two adjacent separators or before a leading one, none after a trailing one. */
static int cg_next_token(const char *s, size_t len, size_t *pos, char sep, size_t *b, size_t *e)
{
    if (*pos >= len) return 0;
    *b = *pos;
    size_t k = *pos;
    while (k < len && s[k] != sep) ++k;
    *e = k;
    *pos = k < len ? k + 1 : k;
    return 1;
}

/* spec -> labels with their group; returns the number of groups or -1 (err set) */
static int cg_parse(const char *spec, int is_long, cg_label_t *lab, int *n_lab, char *err, int err_len)
{
    const size_t len = strlen(spec);
    if (!is_long) /* ref: src/main.cc:396-408 */
        for (size_t i = 0; i < len; ++i) {
            const char a = spec[i];
            if (a != '+' && !(a >= 'a' && a <= 'z') && !(a >= 'A' && a <= 'Z') && !(a >= '0' && a <= '9')) {
                char msg[160];
                snprintf(msg, sizeof msg, "character '%c' not valid chain ID in chain groups, valid characters are [A-z0-9] and '+' as separator", a);
                return cg_fail(err, err_len, msg);
            }
        }
    int n_groups = 0;
    *n_lab = 0;
    size_t pos = 0, gb, ge;
    while (cg_next_token(spec, len, &pos, '+', &gb, &ge)) {
        int in_group = 0;
        if (!is_long) { /* one character per chain (ref: src/main.cc:411-420) */
            for (size_t i = gb; i < ge; ++i) {
                if (*n_lab >= CG_MAX_LABELS) return cg_fail(err, err_len, "too many chain labels");
                memset(lab[*n_lab].label, 0, 4);
                lab[*n_lab].label[0] = spec[i];
                lab[(*n_lab)++].group = n_groups;
                ++in_group;
            }
        } else { /* labels of at most 3 characters between '/' (ref: src/main.cc:427-443) */
            size_t p2 = gb, lb, le;
            while (cg_next_token(spec, ge, &p2, '/', &lb, &le)) {
                if (le - lb > 3) return cg_fail(err, err_len, "Chain labels can not have more than 3 characters");
                /* an empty label names no chain of any structure: the reference refuses every structure */
                if (le == lb) return cg_fail(err, err_len, "empty chain label");
                if (*n_lab >= CG_MAX_LABELS) return cg_fail(err, err_len, "too many chain labels");
                memset(lab[*n_lab].label, 0, 4);
                memcpy(lab[*n_lab].label, spec + lb, le - lb);
                lab[(*n_lab)++].group = n_groups;
                ++in_group;
            }
        }
        /* (an empty group - "A++B", "+A" - is refused for every structure by the reference, src/structure.c:1038) */
        if (in_group == 0) return cg_fail(err, err_len, "empty chain group");
        ++n_groups;
        if (n_groups > 65535) return cg_fail(err, err_len, "too many chain groups");
    }
    for (int i = 0; i < *n_lab; ++i)
        for (int j = 0; j < i; ++j)
            if (memcmp(lab[i].label, lab[j].label, 4) == 0)
                /* (within one group the reference refuses every structure, src/structure.c:1070: the group can never
                   hold as many distinct chains as it names) */
                return cg_fail(err, err_len, lab[i].group == lab[j].group ? "a chain is named twice in one group"
                                                                          : "overlapping groups are not supported");
    return n_groups;
}

/* the call errors of a spec and its flags that need no parse; 0 or -1 (err set) */
static int cg_check(const char *spec, int flags, char *err, int err_len)
{
    if (flags & ~(FREESASA_INGEST_GROUPS_LONG | FREESASA_INGEST_SEPARATE_CHAINS)) return cg_fail(err, err_len, "unknown flags");
    const int separate = (flags & FREESASA_INGEST_SEPARATE_CHAINS) != 0;
    if (separate && spec) return cg_fail(err, err_len, "chain groups and separate chains can't be combined");
    if (!separate && !spec) return cg_fail(err, err_len, "no chain groups given");
    return 0;
}

int freesasa_ingest_chain_groups_parse(const char *spec, int flags, char *labels_out, int32_t *label_group_out, int *n_labels_out,
                                       char *err, int err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (!labels_out || !label_group_out || !n_labels_out) return cg_fail(err, err_len, "null argument");
    *n_labels_out = 0;
    if (cg_check(spec, flags, err, err_len)) return -1;
    if (flags & FREESASA_INGEST_SEPARATE_CHAINS) return 0;
    cg_label_t *lab = (cg_label_t *)hf_malloc(sizeof(cg_label_t) * CG_MAX_LABELS);
    if (!lab) return cg_fail(err, err_len, "out of memory");
    int n_lab = 0;
    const int G = cg_parse(spec, (flags & FREESASA_INGEST_GROUPS_LONG) != 0, lab, &n_lab, err, err_len);
    for (int i = 0; G >= 0 && i < n_lab; ++i) { memcpy(labels_out + 4 * i, lab[i].label, 4); label_group_out[i] = lab[i].group; }
    if (G >= 0) *n_labels_out = n_lab;
    free(lab);
    return G;
}

int freesasa_ingest_chain_groups(const freesasa_ingest_batch *b, const char *spec, int flags, int32_t *group_out,
                                 int32_t *n_groups_out, int32_t *status_out, char *err, int err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (!b || !group_out || !n_groups_out || !status_out) return cg_fail(err, err_len, "null argument");
    if (cg_check(spec, flags, err, err_len)) return -1;
    const int separate = (flags & FREESASA_INGEST_SEPARATE_CHAINS) != 0;
    cg_label_t *lab = NULL;
    int n_lab = 0, G = 0;
    if (!separate) {
        lab = (cg_label_t *)hf_malloc(sizeof(cg_label_t) * CG_MAX_LABELS);
        if (!lab) return cg_fail(err, err_len, "out of memory");
        G = cg_parse(spec, (flags & FREESASA_INGEST_GROUPS_LONG) != 0, lab, &n_lab, err, err_len);
        if (G < 0) { free(lab); return -1; }
    }
    int *present = NULL;
    if (!separate && n_lab > 0) {
        present = (int *)hf_malloc(sizeof(int) * (size_t)n_lab);
        if (!present) { free(lab); return cg_fail(err, err_len, "out of memory"); }
    }
    for (int s = 0; s < b->n_structs; ++s) {
        const int64_t a0 = b->offsets[s], a1 = b->offsets[s + 1];
        const int64_t r0 = b->res_offsets[s], r1 = b->res_offsets[s + 1];
        for (int64_t i = a0; i < a1; ++i) group_out[i] = -1;
        status_out[s] = b->status ? b->status[s] : FREESASA_INGEST_OK;
        n_groups_out[s] = separate ? 0 : G;
        if (status_out[s] != FREESASA_INGEST_OK) continue;
        if (separate) {
            /* a new structure wherever the chain label changes from one atom to the next, a recurring label included
               (ref: freesasa_pdb_get_chains, src/pdb.c:96-140) */
            int g = -1;
            const char *last = NULL;
            for (int64_t r = r0; r < r1; ++r) {
                const char *lbl = b->res_chain + 4 * r;
                if (b->res_first[r + 1] > b->res_first[r] && (!last || memcmp(lbl, last, 4) != 0)) { ++g; last = lbl; }
                for (int64_t i = b->res_first[r]; i < b->res_first[r + 1]; ++i) group_out[i] = g;
            }
            if (g + 1 > 65535) {
                for (int64_t i = a0; i < a1; ++i) group_out[i] = -1;
                status_out[s] = FREESASA_INGEST_EGROUP;
                continue;
            }
            n_groups_out[s] = g + 1;
            continue;
        }
        for (int i = 0; i < n_lab; ++i) present[i] = 0;
        for (int64_t r = r0; r < r1; ++r) {
            if (b->res_first[r + 1] <= b->res_first[r]) continue;
            const char *lbl = b->res_chain + 4 * r;
            int hit = -1;
            for (int i = 0; i < n_lab; ++i) /* (ref: chain_group_has_chain, strncmp over the 4 bytes of a label) */
                if (strncmp(lab[i].label, lbl, 4) == 0) { hit = i; break; }
            if (hit < 0) continue;
            present[hit] = 1;
            for (int64_t i = b->res_first[r]; i < b->res_first[r + 1]; ++i) group_out[i] = lab[hit].group;
        }
        /* every named chain has to be there (ref: src/structure.c:1066-1075) */
        int ok = 1;
        for (int i = 0; i < n_lab; ++i) ok &= present[i];
        if (!ok) {
            for (int64_t i = a0; i < a1; ++i) group_out[i] = -1;
            status_out[s] = FREESASA_INGEST_EGROUP;
        }
    }
    free(lab);
    free(present);
    return 0;
}

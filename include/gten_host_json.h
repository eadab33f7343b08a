/*
 * gten_host_json.h -- a subset of JSON Schema compiled to a pattern of the regex dialect of include/gten_host_regex.h (libgten_host.so,
 * host/capi_text.cpp, host/json_schema.h).  DESIGN.md §3.21.  Device-free.
 *
 * The pattern is a string of that dialect and nothing else: gten_host_fsm_add_regex of it is "emit JSON that fits this schema".  The
 * expansion over the vocabulary then runs on the device as for any pattern, and ending follows the regex rule: an object's closing
 * brace has nothing behind it and is FINAL.
 *
 * What is taken: type (a name or a list) string / integer / number / boolean / null / array / object; minLength, maxLength; items,
 * minItems, maxItems; properties (at most 64, emitted in their order), required, additionalProperties false (absent means the same);
 * enum and const of strings, integers, booleans and null; anyOf, oneOf; $ref to #/$defs/NAME or #/definitions/NAME; no type at all: any
 * JSON value of up to `depth` levels of nesting.  Ignored: title description default examples $schema $id $defs definitions.  Every other
 * key is refused, so that no constraint is dropped silently.  The construction is fixed and written out in host/json_schema.h.
 */
#ifndef GTEN_HOST_JSON_H
#define GTEN_HOST_JSON_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* schema_text: the schema as JSON, NUL-terminated.  ws: 0 compact, 1 an optional space after every `,` and `:`.  depth: 0 .. 4, the
 * nesting of "any value".  Returns the pattern's length; out holds cap bytes and gets the pattern and a NUL when length < cap (nothing is
 * written otherwise: ask with cap 0 first).  Refusals, with a NUL-terminated text in error_out (error_cap bytes, may be NULL / 0):
 *   -1 malformed JSON, the byte offset as decimal text (an empty text: ws or depth out of range, or a null schema);
 *   -4 a key or value outside the subset, the offending key's path, e.g. /properties/age/minimum. */
long long gten_host_json_schema_regex(const char* schema_text, int ws, int depth, char* out, long long cap, char* error_out, long long error_cap);

#ifdef __cplusplus
}
#endif
#endif

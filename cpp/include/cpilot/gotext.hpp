// The small Go standard-library text rules the reference's behaviour rests
// on, each defined once: UTF-8 (unicode/utf8), white space (unicode.IsSpace,
// strings.TrimSpace), strconv.Atoi, hex digits and strconv.ParseFloat as of
// Go 1.9. Templates, durations, the JSON5 reader and user metrics all read
// text through these.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

namespace cpilot {
namespace gotext {

// ---------- UTF-8 ----------

// Append the encoding of cp; the caller has ruled out what must not be
// encoded.
void appendUtf8(std::string& out, uint32_t cp);

// Length in bytes of the well-formed UTF-8 sequence at s[i], 0 if there is
// none (bad lead byte, truncation, overlong form, surrogate, > U+10FFFF).
size_t utf8SeqLen(const std::string& s, size_t i, uint32_t* cpOut = nullptr);

// Strict decode; false on any malformed sequence.
bool decodeUtf8(const std::string& s, std::u32string* out);

// Code points of s for width/precision purposes; a malformed byte counts
// as one, as Go's rune iteration does.
size_t runeCount(const std::string& s);

// ---------- white space ----------

// unicode.IsSpace
bool isSpace(uint32_t cp);

// strings.TrimSpace; a malformed byte is no space and ends the trimming
std::string trimSpace(const std::string& s);

// ---------- numbers ----------

// [+-]?[0-9]+ within int64: what strconv.Atoi accepts
bool atoi(const std::string& s, int64_t* out);

// value of one hex digit, -1 for anything else
int hexVal(char c);

// digits* ('.' digits*)? ([eE][+-]?digits+)?  with a mantissa digit and
// nothing else: no sign, no hex, no underscores, no NUL
bool isDecimalFloat(const std::string& s);

// strconv.ParseFloat(s, 64): an optional sign, then "inf" or "infinity" in
// any case, "nan" in any case (without a sign only), or a decimal float. A
// value that rounds to infinity is out of range: refused.
bool parseFloat(const std::string& s, double* out);

}  // namespace gotext
}  // namespace cpilot

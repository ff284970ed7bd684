// Config template engine: a focused reimplementation of the subset of Go
// text/template that ContainerPilot configs use, rendered against the
// process environment with missingkey=zero semantics, or (Template, for
// watch render files) against a JSON value.
//
// Supported: {{ .VAR }} lookups, {{- -}} whitespace trimming, variables
// with Go 1.9 block scoping ($x := ..., also in if/with/range headers),
// pipelines (a | b | c), nested calls with parens, Go string, number and
// bool constants, if/else if/else, with/else, range/else (one and two
// variables), comments, the Go builtins, and the functions: default, env,
// split, join, replaceAll, regexReplaceAll, loop. Whatever Go would
// refuse, or the engine cannot honour exactly, is an error; the deliberate
// exceptions are listed in COMPONENTS.md.
// Parity: /root/reference/config/template/template.go:19-180.
#pragma once

#include <memory>
#include <string>

#include "cpilot/json.hpp"

namespace cpilot {

// Render `text` against the current process environment.
// Throws std::runtime_error on parse or execution errors.
std::string renderTemplate(const std::string& text);

// A template parsed once and rendered against data: the root "." (and "$")
// is `data` instead of the environment. JSON objects are maps (.A.B,
// $v.Field, `index m "k"`, `len m`), arrays are lists, scalars map as they
// are. A missing key and a field of a non-map both yield "". Every function
// keeps working; `env` still reads the process environment.
// Cheap to copy: copies share the parsed tree.
class Template {
 public:
  // Throws std::runtime_error on a parse error.
  static Template parse(const std::string& text);
  // Throws std::runtime_error on an execution error, or if never parsed.
  std::string render(const Json& data) const;
  bool parsed() const { return impl_ != nullptr; }

 private:
  struct Impl;
  std::shared_ptr<const Impl> impl_;
};

}  // namespace cpilot

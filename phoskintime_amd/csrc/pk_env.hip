// pk_env.hip -- the library's only reads of the process environment: the snapshot of every switch and the reader of the live ones
// (pk_env.hpp says which is which and states the snapshot rule).
#include <cstdlib>
#include "pk_env.hpp"

namespace pk {

const Env& env() {
  static const Env once = env_parse(getenv);
  return once;
}

Env env_live() {
  Env e = env();
  env_parse_live(e, getenv);
  return e;
}

}  // namespace pk

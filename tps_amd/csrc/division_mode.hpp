// How a function divides floating-point numbers is written at the head of its body, never left to what the including unit
// has switched on before (physics_plasma.hpp switches x / y to x * (1 / y) from its namespace to the end of the unit).
//   TPSRHS_IEEE_DIVISION        correctly rounded quotients: what a restatement of the function computes
//   TPSRHS_RECIPROCAL_DIVISION  x * (1 / y), one reciprocal per distinct divisor
// Empty for a compiler other than clang (the sanitizer tests build several of these headers with g++ -Wall -Werror, which
// divides the IEEE way and knows no such pragma).
#ifndef TPSRHS_DIVISION_MODE_HPP_
#define TPSRHS_DIVISION_MODE_HPP_

#if defined(__clang__)
#define TPSRHS_IEEE_DIVISION _Pragma("clang fp reciprocal(off)")
#define TPSRHS_RECIPROCAL_DIVISION _Pragma("clang fp reciprocal(on)")
#else
#define TPSRHS_IEEE_DIVISION
#define TPSRHS_RECIPROCAL_DIVISION
#endif

#endif

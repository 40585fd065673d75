// `spzk serve --socket PATH [--jobs N] [--idle-exit SECONDS] [--with-parent]`: the resident prover process (spzk_serve.cpp)
#pragma once
int spzk_serve_main(int argc, char **argv);
